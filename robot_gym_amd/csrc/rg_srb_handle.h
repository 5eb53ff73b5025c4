// rg_srb_handle.h -- what the translation units of the simulator (rg_srb.hip, rg_srb_terrain.hip, rg_srb_contact.hip) share on the HOST side: the handle of include/rg_srb.h,
// the small helpers of its entry points, and the calls by which rg_srb.hip (the plane) hands a tick, a reset or the end of
// a handle's life over to rg_srb_terrain.hip once a terrain is set.  Private to robot_gym_amd/csrc.  Included after
// rg_host.h and rg_srb_dev.inc (SrbCfg, Obs and DevCfg are the including file's), outside its anonymous namespace.
#ifndef RG_SRB_HANDLE_H
#define RG_SRB_HANDLE_H

constexpr int kSrbBlock = 256;         // 64 robots per workgroup
constexpr int kSrbBodyRows = 19;       // per-robot true body [kSrbBodyRows][B]: mass, I[9], I^-1[9]
constexpr int kSrbResetRows = 5;       // reset staging [kSrbResetRows][B]: robot, x, y, yaw, height

// The ground as the kernels of rg_srb_terrain.hip take it: a validated rg_srb_terrain.  kind 0: the plane.
struct rg_srb_ground {
  int kind = 0, rows = 0, cols = 0;
  double cell = 0.0, amplitude = 0.0, x0 = 0.0, y0 = 0.0;
  unsigned long long seed = 0;
  const long long *key = nullptr;      // [B] device, caller-owned, or NULL
  const double *heights = nullptr;     // [rows][cols] device, caller-owned
};

struct rg_srb_handle {
  SrbCfg c;
  rg_srb_config cfg;
  double cfg_Iinv[9];
  int B = 0, device = 0;
  DevCfg *dcfg = nullptr;     // the kinematic fields of the controller's DevCfg, for leg_fk / leg_ik
  double *body = nullptr;     // [kSrbBodyRows][B]
  double *stage = nullptr;    // [kSrbResetRows][B]
  rg_srb_ground ground;       // rg_srb_set_terrain
  int32_t *reset_mask = nullptr;   // [B], allocated by the first rg_srb_set_terrain: the robots a host reset settles
  std::vector<double> body_host, stage_host;
  std::vector<int32_t> mask_host;
  std::string err;
};

// rg_srb_terrain.hip, for the dispatch of rg_srb_step / rg_srb_reset on a handle whose ground.kind != 0.  Arguments are
// checked by the caller, the device is the caller's DeviceScope.  Nothing synchronises.
int rg_srb_terrain_step_launch(rg_srb_handle *h, double *state, const float *grf, const float *foot_target, const int32_t *desired_state,
                               const double *ext, const rg_srb_obs_ptrs *obs, hipStream_t s);
int rg_srb_terrain_settle_launch(rg_srb_handle *h, double *state, const int32_t *mask, const rg_srb_obs_ptrs *obs, hipStream_t s);

// rg_srb.hip: the text rg_srb_last_error(NULL) returns on this thread (a call that was given no handle)
void rg_srb_thread_error(const char *text);

namespace {

inline int hip_fail(rg_srb_handle *h, const char *what, hipError_t e) { return hip_fail(h, RG_SRB_ERR_HIP, what, e); }
inline int launch_status(rg_srb_handle *h, const char *what) { return launch_status(h, RG_SRB_ERR_HIP, what); }

}  // namespace

#endif /* RG_SRB_HANDLE_H */

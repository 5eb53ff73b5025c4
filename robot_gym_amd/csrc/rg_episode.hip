// rg_episode.hip -- the episode reset on the device of include/rg_episode.h.  Its own translation unit of librg_mpc.so.
//
// Layout: one 64-lane wave per robot, one wave per workgroup, in both kernels, so every branch around a cross-lane
// operation or a __syncthreads is uniform over the workgroup.  A robot whose mask is 0 leaves after a load (the plan
// kernel also clears the robot's stale flag in reset_mask_out when it is set).
//
// rg_episode_plan_kernel: the target and the descent are computed by every lane (uniform values); at each descent step
// lane m & 7 evaluates the potential of neighbour m and the choice is made over lanes 0..7 in MOTION order.  Way points and
// their cumulative length go to LDS.  The path points are interpolated one per lane in chunks of 64; the arc-length table
// is the IN-ORDER sum arc_table forms, done as a serial chain over the chunk's 64 segment lengths read lane by lane (a
// parallel scan rounds differently).  first_same_x compares each point with every earlier one, 64 per load, lane by lane.
// rg_episode_reset_kernel: lanes 0..3 run the simulator's reset for their leg (srb_reset_robot of rg_srb_dev.inc), then
// the wave observes the path (goto_observe of rg_goto_dev.inc).  rg_episode_ctl_reset_kernel is the controller's masked
// reset (rg_mpc_reset_masked), one thread per robot: it lives here because the kernel sets of rg_mpc.hip and
// rg_mpc_state.hip are pinned.
// The simulator's configuration and the obstacles are read from device memory, not from the kernel arguments.
// LDS: plan kernel 3 * 64 + 2 * 16 doubles + 2 * 8 ints = 1856 bytes; reset kernel 5 * 128 doubles = 5120 bytes.
//
// Parity: tests/episode_model.py (the target stream; plan_path / build_path of goto_path.py).  Contraction is off.  What
// remains different from numpy: hypot (plan only, see rg_episode.h) and the atan2 / sincos of the start heading.
#include <hip/hip_runtime.h>
#include <math.h>
#include <climits>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>
#include "../../include/rg_episode.h"
#include "rg_host.h"

#pragma clang fp contract(off)

#include "rg_mpc_dev.h"
#include "rg_mpc_state.h"

namespace {

#include "rg_srb_dev.inc"
#include "rg_goto_dev.inc"

constexpr int kMaxWay = RG_EPISODE_MAX_WAYPOINTS;
constexpr int kMaxObs = RG_EPISODE_MAX_OBSTACLES;
constexpr int kMaxOsc = RG_EPISODE_MAX_OSCILLATION;
constexpr int kAccBlock = 256;

struct EpCfg {
  int B, n_max, nobs, osc, max_way, ncp;
  double half_kp, half_eta, half_area, grid, radius, inv_radius, spacing, body_height;
  unsigned long long seed;
};

// what the kernels read from device memory instead of their arguments (scalar registers are short in both)
struct EpDev {
  SrbCfg sc;
  double ox[kMaxObs], oy[kMaxObs];   // the obstacles; without any, the planner's dummy one
};

#include "rg_stream_dev.inc"

// one coordinate of the target stream (rg_episode.h, a.)
__device__ __forceinline__ double draw_coord(unsigned long long seed, unsigned long long key, unsigned long long episode,
                                             unsigned long long attempt, unsigned long long axis) {
  const double u = unit53(mix_word(mix_word(mix_word(mix_word(seed, key), episode), attempt), axis));
  const double v = -2.5 + 5.0 * u;
  double c = rint(100.0 * v);
  if (c > 0.0 && c < 100.0) c = 100.0;
  if (c < 0.0 && c > -100.0) c = -100.0;
  return (c + 0.0) / 100.0;
}

// hypot with the larger magnitude first.  The library's hypot forms fma(a, a, b * b) from its arguments in the order given, so
// hypot(x, y) and hypot(y, x) can differ in the last bit; numpy's are equal.  Two cells mirrored about the diagonal through
// the target have equal potentials in plan_path and the first in MOTION order wins: ordered arguments keep that tie a tie.
__device__ __forceinline__ double hypot_sym(double x, double y) {
  x = fabs(x); y = fabs(y);
  return x >= y ? hypot(x, y) : hypot(y, x);
}

__device__ __forceinline__ double min3(double a, double b, double c) { a = b < a ? b : a; return c < a ? c : a; }   // Python's min(a, b, c)
__device__ __forceinline__ double max3(double a, double b, double c) { a = b > a ? b : a; return c > a ? c : a; }

// the plan kernel's pointers, passed as one struct so that each is loaded where it is used and not held from the entry
struct PlanPtrs {
  const EpDev *dv;
  const int *mask;
  const double *targets;
  double *ep, *task, *x, *y, *s;
  int *fsx;
  double *hdr;
  const float *obs;
  float *final_obs;
  int *ok;
};

__global__ void __launch_bounds__(kWave) rg_episode_plan_kernel(const EpCfg c, const PlanPtrs a) {
  __shared__ double wpx[kMaxWay], wpy[kMaxWay], wps[kMaxWay];   // way points and their cumulative length
  __shared__ double obx[kMaxObs], oby[kMaxObs];
  __shared__ int pcx[kMaxOsc], pcy[kMaxOsc];                    // the last cells of the descent
  const int b = blockIdx.x, lane = threadIdx.x;
  if (a.mask[b] == 0) {   // uniform over the workgroup
    if (lane == 0 && a.ok[b] != 0) a.ok[b] = 0;
    return;
  }
  const size_t sB = (size_t)c.B;
  const double inf = __builtin_inf();
  if (lane < 2 * c.ncp) a.final_obs[lane * sB + b] = a.obs[lane * sB + b];
  if (lane < c.nobs) { obx[lane] = a.dv->ox[lane]; oby[lane] = a.dv->oy[lane]; }
  __syncthreads();
  // a. target
  const unsigned long long key = word_of(a.ep[RG_EPISODE_ROW_KEY * sB + b]);
  const double episode = a.ep[RG_EPISODE_ROW_EPISODE * sB + b];
  double gx = a.targets ? a.targets[b] : __builtin_nan(""), gy = a.targets ? a.targets[sB + b] : __builtin_nan("");
  if (gx != gx || gy != gy) {
    const unsigned long long e = word_of(episode);
    #pragma unroll 1
    for (unsigned long long attempt = 0; attempt < 64; attempt++) {
      gx = draw_coord(c.seed, key, e, attempt, 0);
      gy = draw_coord(c.seed, key, e, attempt, 1);
      if (gx != 0.0 || gy != 0.0) break;
    }
  }
  int status = RG_EPISODE_PLAN_OK, nway = 0, n = 0;
  double length = 0.0;
  if (!(isfinite(gx) && isfinite(gy))) status = RG_EPISODE_PLAN_TARGET;
  if (status == RG_EPISODE_PLAN_OK) {   // uniform
    // b. plan: the grid of _potential_map
    double lox = obx[0], hix = obx[0], loy = oby[0], hiy = oby[0];
    #pragma unroll 1
    for (int k = 1; k < c.nobs; k++) {
      lox = obx[k] < lox ? obx[k] : lox; hix = obx[k] > hix ? obx[k] : hix;
      loy = oby[k] < loy ? oby[k] : loy; hiy = oby[k] > hiy ? oby[k] : hiy;
    }
    const double reso = c.grid;
    const double minx = min3(lox, 0.0, gx) - c.half_area, miny = min3(loy, 0.0, gy) - c.half_area;
    const double maxx = max3(hix, 0.0, gx) + c.half_area, maxy = max3(hiy, 0.0, gy) + c.half_area;
    const double fxw = rint((maxx - minx) / reso), fyw = rint((maxy - miny) / reso);
    const int xw = fxw < 1e9 ? (int)fxw : 1000000000, yw = fyw < 1e9 ? (int)fyw : 1000000000;
    double d = hypot_sym(0.0 - gx, 0.0 - gy);
    const double fix = rint((0.0 - minx) / reso), fiy = rint((0.0 - miny) / reso);
    int ix = fix < 1e9 ? (int)fix : 1000000000, iy = fiy < 1e9 ? (int)fiy : 1000000000;
    const int m = lane & 7;
    const int mx = (0x5A21 >> (2 * m)) & 3, my = (0x6684 >> (2 * m)) & 3;   // MOTION, two bits per entry: 0 -> 0, 1 -> +1, 2 -> -1
    const int dxm = mx == 2 ? -1 : mx, dym = my == 2 ? -1 : my;
    if (lane == 0) { wpx[0] = 0.0; wpy[0] = 0.0; }
    nway = 1;
    int nprev = 0;
    while (d >= reso) {
      if (nway + 2 > c.max_way) { status = RG_EPISODE_PLAN_WAYPOINTS; break; }   // this cell and the target would not fit
      const int inx = ix + dxm, iny = iy + dym;
      double p = inf;
      if (inx >= 0 && iny >= 0 && inx < xw && iny < yw) {
        const double x = (double)inx * reso + minx, y = (double)iny * reso + miny;
        p = c.half_kp * hypot_sym(x - gx, y - gy);
        double dmin = inf;
        #pragma unroll 1
        for (int k = 0; k < c.nobs; k++) {
          const double dk = hypot_sym(x - obx[k], y - oby[k]);
          dmin = dmin >= dk ? dk : dmin;
        }
        if (dmin <= c.radius) {
          const double dq = dmin <= 0.1 ? 0.1 : dmin;
          const double t = 1.0 / dq - c.inv_radius;
          p = p + c.half_eta * (t * t);
        }
      }
      double minp = inf;
      int best = -1;
#pragma unroll
      for (int k = 0; k < 8; k++) {
        const double pk = __shfl(p, k);
        if (minp > pk) { minp = pk; best = k; }
      }
      if (best < 0) { status = RG_EPISODE_PLAN_WAYPOINTS; break; }
      ix = __shfl(inx, best);
      iy = __shfl(iny, best);
      const double xp = (double)ix * reso + minx, yp = (double)iy * reso + miny;
      d = hypot_sym(gx - xp, gy - yp);
      if (lane == 0) { wpx[nway] = xp; wpy[nway] = yp; }
      nway++;
      // previous.append; pop(0) past oscillation_length; stop on a repeat among them
      // (the cells kept from before hold no repeat among themselves: the loop would have stopped there)
      bool repeat = false;
      #pragma unroll 1
      for (int k = nprev == c.osc ? 1 : 0; k < nprev; k++) repeat = repeat || (pcx[k] == ix && pcy[k] == iy);
      __syncthreads();
      if (lane == 0) {
        if (nprev == c.osc) {
          #pragma unroll 1
          for (int k = 1; k < nprev; k++) { pcx[k - 1] = pcx[k]; pcy[k - 1] = pcy[k]; }
          pcx[nprev - 1] = ix; pcy[nprev - 1] = iy;
        } else { pcx[nprev] = ix; pcy[nprev] = iy; }
      }
      if (nprev < c.osc) nprev++;
      __syncthreads();
      if (repeat) break;
    }
    if (status == RG_EPISODE_PLAN_OK) {
      if (lane == 0) { wpx[nway] = gx; wpy[nway] = gy; }
      nway++;
    }
  }
  __syncthreads();
  if (status == RG_EPISODE_PLAN_OK) {
    // arc_table of the way points: the in-order sum, segment j read from lane j
    double seg = 0.0;
    if (lane >= 1 && lane < nway) {
      const double ddx = wpx[lane] - wpx[lane - 1], ddy = wpy[lane] - wpy[lane - 1];
      seg = sqrt(ddx * ddx + ddy * ddy);
    }
    double acc = 0.0, mine = 0.0;
    #pragma unroll 1
    for (int j = 1; j < nway; j++) {
      acc = acc + __shfl(seg, j);
      if (lane == j) mine = acc;
    }
    if (lane < nway) wps[lane] = mine;
    length = acc;
    const double q = length / c.spacing;
    n = q < 1e9 ? (int)q : INT_MAX;   // a NaN gives INT_MAX, refused below
    if (n < 2) status = RG_EPISODE_PLAN_SHORT;
    else if (n > c.n_max) status = RG_EPISODE_PLAN_LONG;
  }
  __syncthreads();
  if (status != RG_EPISODE_PLAN_OK) {   // uniform: nothing of the robot is reset
    if (lane == 0) { a.ep[RG_EPISODE_ROW_PLAN_STATUS * sB + b] = (double)status; a.ok[b] = 0; }
    return;
  }
  // c. path: interpolate_points, arc_table, first_same_x
  const size_t row = (size_t)b * c.n_max;
  const int last = nway - 1;
  const double wlen = length, step = wlen / (double)(n - 1);
  double carry_x = 0.0, carry_y = 0.0, sacc = 0.0;
  int npts = 0;
  for (int base = 0; base < n; base += kWave) {
    const int i = base + lane;
    const double t = (double)i * step;
    const bool valid = i < n && !(t > wlen + 1e-6);
    double x = 0.0, y = 0.0;
    if (valid) {
      if (t >= wps[last]) { x = wpx[last]; y = wpy[last]; }
      else {
        int k = 0;
        while (k < last - 1 && !(t < wps[k + 1])) k++;
        const double fr = (t - wps[k]) / (wps[k + 1] - wps[k]);
        x = wpx[k] + fr * (wpx[k + 1] - wpx[k]);
        y = wpy[k] + fr * (wpy[k + 1] - wpy[k]);
      }
      a.x[row + i] = x; a.y[row + i] = y;
    }
    const unsigned long long vm = __ballot(valid);   // a prefix of the lanes: t grows with i
    const int cnt = __popcll(vm);
    double qx = __shfl_up(x, 1), qy = __shfl_up(y, 1);
    if (lane == 0) { qx = carry_x; qy = carry_y; }
    const double ddx = x - qx, ddy = y - qy;
    const double dseg = (valid && i > 0) ? sqrt(ddx * ddx + ddy * ddy) : 0.0;
    double smine = 0.0;
    #pragma unroll 1
    for (int j = 0; j < cnt; j++) {
      sacc = sacc + __shfl(dseg, j);
      if (lane == j) smine = sacc;
    }
    if (valid) a.s[row + i] = smine;
    if (cnt > 0) { carry_x = __shfl(x, cnt - 1); carry_y = __shfl(y, cnt - 1); }
    npts += cnt;
    if (cnt < kWave) break;
  }
  __syncthreads();   // the wave's own stores of X are visible to its loads below
  for (int base = 0; base < npts; base += kWave) {
    const int i = base + lane;
    const bool valid = i < npts;
    const double xi = valid ? a.x[row + i] : 0.0;
    int fs = -1;
    #pragma unroll 1
    for (int cb = 0; cb <= base; cb += kWave) {
      const double xj = cb + lane < npts ? a.x[row + cb + lane] : 0.0;
      const int lim = npts - cb < kWave ? npts - cb : kWave;
      #pragma unroll 1
      for (int j = 0; j < lim; j++) {
        const double v = __shfl(xj, j);
        if (fs < 0 && cb + j <= i && v == xi) fs = cb + j;
      }
    }
    if (valid) a.fsx[row + i] = fs < 0 ? i : fs;
  }
  // e. latch the episode that ended, zero the task column, write the header
  if (lane == 0) {
    a.ep[RG_EPISODE_ROW_LAST_RETURN * sB + b] = a.ep[RG_EPISODE_ROW_RETURN * sB + b];
    a.ep[RG_EPISODE_ROW_LAST_LENGTH * sB + b] = a.ep[RG_EPISODE_ROW_LENGTH * sB + b];
    a.ep[RG_EPISODE_ROW_LAST_REASON * sB + b] = a.task[RG_GOTO_ROW_REASON * sB + b];
    a.ep[RG_EPISODE_ROW_RETURN * sB + b] = 0.0;
    a.ep[RG_EPISODE_ROW_LENGTH * sB + b] = 0.0;
    a.ep[RG_EPISODE_ROW_ENDED * sB + b] = 0.0;
    a.ep[RG_EPISODE_ROW_EPISODE * sB + b] = episode + 1.0;
    a.ep[RG_EPISODE_ROW_PLAN_STATUS * sB + b] = 0.0;
    a.ep[RG_EPISODE_ROW_NPTS * sB + b] = (double)npts;
    a.ep[RG_EPISODE_ROW_NWAY * sB + b] = (double)nway;
    a.hdr[b] = (double)npts; a.hdr[sB + b] = sacc; a.hdr[2 * sB + b] = gx; a.hdr[3 * sB + b] = gy;
    a.ok[b] = 1;
  }
  __syncthreads();   // lane 0 has read done_reason
  if (lane < RG_GOTO_STATE_ROWS) a.task[lane * sB + b] = 0.0;
}

__global__ void __launch_bounds__(kWave) rg_episode_reset_kernel(const DevCfg *__restrict__ kc, const EpDev *__restrict__ dv, GotoCfg c, const int *__restrict__ ok,
                                                                double *__restrict__ task, double *__restrict__ sim, Obs o, Paths P,
                                                                float *__restrict__ obs) {
  __shared__ double vx[kMaxVis], vy[kMaxVis];                 // visible points, robot frame, path order
  __shared__ double cx[kMaxVis], cy[kMaxVis], cs[kMaxVis];    // the chain and its cumulative length
  const int b = blockIdx.x, lane = threadIdx.x;
  if (ok[b] == 0) return;   // uniform over the workgroup
  int n = (int)P.hdr[b];
  n = n > c.n_max ? c.n_max : n;
  const double *X = P.x + (size_t)b * c.n_max, *Y = P.y + (size_t)b * c.n_max;
  // start_xy and start_angle of build_path
  const double x0 = X[0], y0 = Y[0];
  double ux = X[1] - x0, uy = Y[1] - y0;
  const double norm = sqrt(ux * ux + uy * uy);
  if (norm > 0.0) { ux = ux / norm; uy = uy / norm; } else { ux = 1.0; uy = 0.0; }
  double ang = atan2(uy, ux);
  if (ang < 0.0) ang = ang + 2 * 3.141592653589793;
  // the pose the task reads back from the simulator's state: p and the yaw of the quaternion (0, 0, sin(ang / 2), cos(ang / 2))
  double sn_h, cs_h;
  sincos(0.5 * ang, &sn_h, &cs_h);
  const double yaw = yaw_of_quat(0.0, 0.0, sn_h, cs_h);
  double bd;
  int bi, bpi;
  goto_observe(c, b, lane, n, task, X, Y, x0, y0, yaw, 0.0, 0.0, 0.0, obs, vx, vy, cx, cy, cs, bd, bi, bpi);
  // the simulator's reset last (it reads nothing the observation wrote): fewer values are held across it
  if (lane < 4) srb_reset_robot(kc, dv->sc, o, sim, b, lane, x0, y0, ang, dv->sc.body_height);   // no cross-lane operation inside
}

__global__ void __launch_bounds__(kAccBlock) rg_episode_accumulate_kernel(int B, double *__restrict__ ep, const float *__restrict__ reward,
                                                                          const int *__restrict__ done) {
  const int b = blockIdx.x * kAccBlock + threadIdx.x;
  if (b >= B) return;
  const size_t sB = (size_t)B;
  if (ep[RG_EPISODE_ROW_ENDED * sB + b] != 0.0) return;
  ep[RG_EPISODE_ROW_RETURN * sB + b] = ep[RG_EPISODE_ROW_RETURN * sB + b] + (double)reward[b];
  ep[RG_EPISODE_ROW_LENGTH * sB + b] = ep[RG_EPISODE_ROW_LENGTH * sB + b] + 1.0;
  if (done[b] != 0) ep[RG_EPISODE_ROW_ENDED * sB + b] = 1.0;
}

thread_local std::string g_create_err;

}  // namespace

// rg_reset_kernel's work for the robots a device mask names (rg_mpc_reset_masked; launcher declared in rg_mpc_state.h)
__global__ void __launch_bounds__(256) rg_episode_ctl_reset_kernel(const DevCfg *__restrict__ c, const DevState st, const int *__restrict__ mask,
                                                                   const double t0, const int B) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B || mask[b] == 0) return;
#define RG_RESET_T0 t0
#include "rg_reset_body.inc"
#undef RG_RESET_T0
}

hipError_t rg_state_reset_masked(const DevCfg *cfg_dev, const DevState &st, int B, const int *mask, double t0, hipStream_t s) {
  hipLaunchKernelGGL(rg_episode_ctl_reset_kernel, dim3(((unsigned)B + 255) / 256), dim3(256), 0, s, cfg_dev, st, mask, t0, B);
  return hipGetLastError();
}

struct rg_episode_handle {
  EpCfg c{};
  EpDev dv{};
  GotoCfg gc{};
  int B = 0, device = 0;
  DevCfg *dcfg = nullptr;   // the kinematic fields of the controller's DevCfg, for leg_fk / leg_ik
  EpDev *dev_cfg = nullptr;
  std::string err;
};

namespace {

bool validate(const rg_episode_config *cfg, std::string &err) {
  char msg[200];
  const RealField reals[] = {{"kp", &cfg->kp, 1, kPositive}, {"eta", &cfg->eta, 1, kFinite}, {"area_width", &cfg->area_width, 1, kPositive},
                             {"grid", &cfg->grid, 1, kPositive}, {"robot_radius", &cfg->robot_radius, 1, kPositive}, {"spacing", &cfg->spacing, 1, kPositive}};
  if (!check_abi("config.", cfg->abi_version, RG_EPISODE_ABI_VERSION, err) || !check_reserved("config.", "reserved0", cfg->reserved0, err) ||
      !check_reserved("config.", "reserved1", cfg->reserved1, err) || !check_reals("config.", reals, err))
    return false;
  if (cfg->eta < 0) { snprintf(msg, sizeof(msg), "config.eta: %g must be >= 0", cfg->eta); err = msg; return false; }
  const IntField ints[] = {{"oscillation_length", cfg->oscillation_length, 1, RG_EPISODE_MAX_OSCILLATION},
                           {"max_waypoints", cfg->max_waypoints, 2, RG_EPISODE_MAX_WAYPOINTS},
                           {"num_obstacles", cfg->num_obstacles, 0, RG_EPISODE_MAX_OBSTACLES}};
  if (!check_ints("config.", ints, err)) return false;
  for (int k = 0; k < RG_EPISODE_MAX_OBSTACLES; k++)
    for (int a = 0; a < 2; a++)
      if (!std::isfinite(cfg->obstacles[k][a])) {
        snprintf(msg, sizeof(msg), "config.obstacles[%d][%d]: %g is not finite", k, a, cfg->obstacles[k][a]);
        err = msg;
        return false;
      }
  return true;
}

int hip_fail(rg_episode_handle *h, const char *what, hipError_t e) { return hip_fail(h, RG_EPISODE_ERR_HIP, what, e); }
int no_device(rg_episode_handle *h) { return no_device(h, RG_EPISODE_ERR_NO_DEVICE, "RG_EPISODE"); }
int launch_status(rg_episode_handle *h, const char *what) { return launch_status(h, RG_EPISODE_ERR_HIP, what); }
int null_arg(rg_episode_handle *h, const char *call, const char *name) { return null_arg(h, RG_EPISODE_ERR_INVALID, call, name); }

}  // namespace

extern "C" {

int32_t rg_episode_abi_version(void) { return RG_EPISODE_ABI_VERSION; }
int32_t rg_episode_config_size(void) { return (int32_t)sizeof(rg_episode_config); }
int32_t rg_episode_state_rows(void) { return RG_EPISODE_ROWS; }
const char *rg_episode_last_error(const rg_episode_handle *h) { return h ? h->err.c_str() : g_create_err.c_str(); }

int rg_episode_create(const rg_episode_config *ecfg, const rg_srb_config *scfg, const rg_goto_config *gcfg, int32_t batch, int32_t device,
                      rg_episode_handle **out) {
  if (!ecfg || !scfg || !gcfg || !out) { g_create_err = "create: null config or out"; return RG_EPISODE_ERR_INVALID; }
  *out = nullptr;
  std::string err;
  double Iinv[9];
  if (!check_batch(batch, RG_EPISODE_MAX_BATCH, err) || !validate(ecfg, err)) { g_create_err = err; return RG_EPISODE_ERR_INVALID; }
  if (!srb_validate(scfg, batch, Iinv, err)) { g_create_err = "srb " + err; return RG_EPISODE_ERR_INVALID; }
  if (!goto_validate(gcfg, batch, err)) { g_create_err = "goto " + err; return RG_EPISODE_ERR_INVALID; }
  rg_episode_handle *h = new rg_episode_handle();
  h->B = batch;
  h->device = device;
  EpCfg &c = h->c;
  c.B = batch; c.n_max = gcfg->n_max; c.osc = ecfg->oscillation_length; c.max_way = ecfg->max_waypoints; c.ncp = gcfg->num_cam_pts;
  c.half_kp = 0.5 * ecfg->kp; c.half_eta = 0.5 * ecfg->eta; c.half_area = ecfg->area_width / 2.0; c.grid = ecfg->grid;
  c.radius = ecfg->robot_radius; c.inv_radius = 1.0 / ecfg->robot_radius; c.spacing = ecfg->spacing; c.body_height = scfg->body_height;
  c.seed = ecfg->seed;
  c.nobs = ecfg->num_obstacles;
  for (int k = 0; k < c.nobs; k++) { h->dv.ox[k] = ecfg->obstacles[k][0]; h->dv.oy[k] = ecfg->obstacles[k][1]; }
  if (c.nobs == 0) { c.nobs = 1; h->dv.ox[0] = h->dv.oy[0] = ecfg->area_width + 1.0; }   // plan_path's dummy obstacle, outside the area
  srb_fill_cfg(scfg, batch, h->dv.sc);
  goto_fill_cfg(gcfg, batch, h->gc);
  if (device == RG_EPISODE_DEVICE_NONE) {   // a host-only handle: the configuration, for argument checks on any machine
    *out = h;
    return RG_EPISODE_OK;
  }
  std::optional<DeviceScope> dev;
  if (const int rc = enter_device(device, &dev, RG_EPISODE_ERR_NO_DEVICE, RG_EPISODE_ERR_INVALID, RG_EPISODE_ERR_HIP, g_create_err)) { delete h; return rc; }
  DevCfg *kin = new DevCfg();
  srb_fill_kinematics(scfg, kin);
  hipError_t e = hipMalloc((void **)&h->dcfg, sizeof(DevCfg));
  if (e == hipSuccess) e = hipMalloc((void **)&h->dev_cfg, sizeof(EpDev));
  if (e != hipSuccess) {
    g_create_err = std::string("hipMalloc failed: ") + hipGetErrorString(e);
    delete kin;
    rg_episode_destroy(h);
    return RG_EPISODE_ERR_ALLOC;
  }
  e = hipMemcpy(h->dcfg, kin, sizeof(DevCfg), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(h->dev_cfg, &h->dv, sizeof(EpDev), hipMemcpyHostToDevice);
  delete kin;
  if (e != hipSuccess) {
    g_create_err = std::string("hipMemcpy failed: ") + hipGetErrorString(e);
    rg_episode_destroy(h);
    return RG_EPISODE_ERR_HIP;
  }
  *out = h;
  return RG_EPISODE_OK;
}

void rg_episode_destroy(rg_episode_handle *h) {
  if (!h) return;
  if (h->device >= 0) {
    DeviceScope dev(h->device);
    if (h->dcfg) (void)hipFree(h->dcfg);
    if (h->dev_cfg) (void)hipFree(h->dev_cfg);
  }
  delete h;
}

int rg_episode_reset(rg_episode_handle *h, const int32_t *mask, const double *targets, double *episode_state, double *task_state,
                     double *sim_state, const rg_srb_obs_ptrs *sim_obs, const rg_goto_path_ptrs *paths, float *obs, float *final_obs,
                     int32_t *reset_mask_out, void *stream) {
  if (!h) { g_create_err = "reset: null handle"; return RG_EPISODE_ERR_INVALID; }
  RG_NEED("reset", mask, "mask");
  RG_NEED("reset", episode_state, "episode_state");
  RG_NEED("reset", task_state, "task_state");
  RG_NEED("reset", sim_state, "sim_state");
  RG_NEED("reset", obs_ok(sim_obs), "sim_obs pointer");
  RG_NEED("reset", paths_ok(paths), "paths pointer");
  RG_NEED("reset", obs, "obs");
  RG_NEED("reset", final_obs, "final_obs");
  RG_NEED("reset", reset_mask_out, "reset_mask_out");
  if (reset_mask_out == mask) { h->err = "reset: reset_mask_out must not alias mask"; return RG_EPISODE_ERR_INVALID; }
  if (h->device < 0) return no_device(h);
  DeviceScope dev(h->device);
  if (dev.err != hipSuccess) return hip_fail(h, "hipSetDevice failed", dev.err);
  hipStream_t s = (hipStream_t)stream;
  const PlanPtrs pp{h->dev_cfg, mask, targets, episode_state, task_state, paths->x, paths->y, paths->s, paths->first_same_x, paths->hdr, obs, final_obs,
                    reset_mask_out};
  hipLaunchKernelGGL(rg_episode_plan_kernel, dim3((unsigned)h->B), dim3(kWave), 0, s, h->c, pp);
  int rc = launch_status(h, "rg_episode_plan_kernel launch");
  if (rc) return rc;
  hipLaunchKernelGGL(rg_episode_reset_kernel, dim3((unsigned)h->B), dim3(kWave), 0, s, h->dcfg, h->dev_cfg, h->gc, reset_mask_out, task_state, sim_state,
                     to_obs(sim_obs), to_paths(paths), obs);
  return launch_status(h, "rg_episode_reset_kernel launch");
}

int rg_episode_accumulate(rg_episode_handle *h, double *episode_state, const float *reward, const int32_t *done, void *stream) {
  if (!h) { g_create_err = "accumulate: null handle"; return RG_EPISODE_ERR_INVALID; }
  RG_NEED("accumulate", episode_state, "episode_state");
  RG_NEED("accumulate", reward, "reward");
  RG_NEED("accumulate", done, "done");
  if (h->device < 0) return no_device(h);
  DeviceScope dev(h->device);
  if (dev.err != hipSuccess) return hip_fail(h, "hipSetDevice failed", dev.err);
  hipLaunchKernelGGL(rg_episode_accumulate_kernel, dim3(((unsigned)h->B + kAccBlock - 1) / kAccBlock), dim3(kAccBlock), 0, (hipStream_t)stream, h->B,
                     episode_state, reward, done);
  return launch_status(h, "rg_episode_accumulate_kernel launch");
}

}  // extern "C"

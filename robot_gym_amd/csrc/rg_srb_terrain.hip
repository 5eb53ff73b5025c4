// rg_srb_terrain.hip -- the heightfield ground of include/rg_srb.h: the tick on it, settle and the height query (the ground
// function itself is rg_srb_ground.inc, shared with the measured-contact tick of rg_srb_contact.hip).  Its own translation
// unit of librg_mpc.so, so that rg_srb.hip keeps reporting exactly its two kernels.
//
// Layout: that of rg_srb.hip.  The step kernel stands on the shared body of a tick (rg_srb_tick.inc, where the cross-lane
// operations and their invariants are stated) and owns step 1 and the fall clearance with the ground function where the
// plane has the literal 0: lane = (robot, leg), float64, no LDS.  The ground is asked at two points outside
// the sub-step loop (a landing foot; the fall test), each a few dozen 64-bit integer operations (random: seven mix rounds
// for the four vertices of a cell, the prefix over (key, I) shared) or four loads (grid).  The settle kernel computes all
// four foot heights in every lane, so it needs no shuffle, and loads everything before it stores: the four lanes of a robot
// share a wave, and leg 0 writes the p.z the others read.
//
// Parity: tests/terrain_model.py restates the ground function, the three changed rules and settle in float64 numpy.
// Floating-point contraction is off for the whole file, the controller's leg_fk / leg_ik included.
#include <hip/hip_runtime.h>
#include <math.h>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>
#include "../../include/rg_srb.h"
#include "rg_host.h"

#pragma clang fp contract(off)

#include "rg_mpc_dev.h"

namespace {

#include "rg_srb_dev.inc"

}  // namespace

#include "rg_srb_handle.h"

namespace {

constexpr int kBlock = kSrbBlock;

// sum4 and the tick_* functions, the body of a tick: shared with the other three step kernels
#include "rg_srb_tick.inc"

// kCoordBound, the hash chain and Ground, h(x, y; robot) of rg_srb.h: shared with rg_srb_contact.hip
#include "rg_srb_ground.inc"

// One control tick on the ground g.  Its own: the schedule's step 1 with a landing foot put on the ground under it, the
// commanded force through every stance foot, and the body's height above the ground under it as the clearance of the fall test.
__global__ void __launch_bounds__(kBlock) rg_srb_terrain_step_kernel(const DevCfg *__restrict__ kc, SrbCfg c, rg_srb_ground g,
                                                                      const double *__restrict__ body, double *__restrict__ state,
                                                                      const float *__restrict__ grf, const float *__restrict__ foot_target,
                                                                      const int *__restrict__ desired, const double *__restrict__ ext, Obs o) {
  const int t = blockIdx.x * kBlock + threadIdx.x;
  const Ground ground{g};
  const int leg = t & 3;
  const bool in_batch = (t >> 2) < c.B;
  const int b = in_batch ? (t >> 2) : c.B - 1;   // lanes past the batch compute on the last robot and store nothing
  const size_t sB = (size_t)c.B;
  double p[3], qt[4], v[3], w[3], foot[3], q[3], stance, steps, I[9], Iinv[9], eF[3], eT[3];
  const bool running = tick_load_state(state, sB, b, leg, p, qt, v, w, foot, q, stance, steps);
  const double mass = tick_load_body(body, sB, b, I, Iinv);
  double R[9];
  quat_rot(qt, R);
  // 1. feet
  const bool swing = desired[(size_t)b * 4 + leg] == 0 /* RG_LEG_SWING */;
  double fbody[3] = {0.0, 0.0, 0.0};
  if (swing) {
    const double ft[3] = {foot_target[(size_t)b * 12 + 3 * leg], foot_target[(size_t)b * 12 + 3 * leg + 1], foot_target[(size_t)b * 12 + 3 * leg + 2]};
    double r[3];
    rot(R, ft, r);
    foot[0] = p[0] + r[0]; foot[1] = p[1] + r[1]; foot[2] = p[2] + r[2];
    stance = 0.0;
  } else {
    if (stance == 0.0) { foot[2] = ground(b, foot[0], foot[1]); stance = 1.0; }
#pragma unroll
    for (int i = 0; i < 3; i++) fbody[i] = -(double)grf[(size_t)b * 12 + 3 * leg + i];
  }
  tick_load_ext(ext, sB, b, eF, eT);
  const double dt = c.dt, wz = mass * -c.g;
  // 2. sub-steps
  for (int s = 0; s < c.substeps; s++) {
    double f[3], F[3], T[3];
    quat_rot(qt, R);
    rot(R, fbody, f);
    tick_wrench(f, foot, p, eF, eT, wz, F, T);
    tick_body(R, I, Iinv, mass, dt, F, T, w, v, p);
    tick_quat(dt, w, qt);
  }
  steps = steps + (double)c.substeps;
  // 3. fall, and the stores
  const int bad = tick_bad(p, qt, v, w, foot);
  const bool store = tick_store(state, c, b, leg, in_batch && running, bad, p[2] - ground(b, p[0], p[1]), p, qt, v, w, foot, stance, steps);
  // 4. observation
  write_obs(kc, c, o, state, b, leg, store, p, qt, v, w, foot, q, stance, steps, 1);
}

// Settle of rg_srb.h: lane = (robot, leg).  flat: the handle has no terrain and every height is 0.0.
__global__ void __launch_bounds__(kBlock) rg_srb_terrain_settle_kernel(const DevCfg *__restrict__ kc, SrbCfg c, rg_srb_ground g, int flat,
                                                                        double *state, const int *__restrict__ mask, Obs o) {
  const int t = blockIdx.x * kBlock + threadIdx.x;
  const int leg = t & 3;
  const bool in_batch = (t >> 2) < c.B;
  const int b = in_batch ? (t >> 2) : c.B - 1;
  const size_t sB = (size_t)c.B;
  const Ground ground{g};
  // every load comes before the first store (leg 0 writes the p.z the other three lanes of the robot read)
  double p[3], qt[4], v[3], w[3], foot[3], q[3], hs[4];
#pragma unroll
  for (int i = 0; i < 3; i++) {
    p[i] = state[(RG_SRB_ROW_P + i) * sB + b];
    v[i] = state[(RG_SRB_ROW_V + i) * sB + b];
    w[i] = state[(RG_SRB_ROW_W + i) * sB + b];
    foot[i] = state[(RG_SRB_ROW_FOOT + 3 * leg + i) * sB + b];
    q[i] = state[(RG_SRB_ROW_Q + 3 * leg + i) * sB + b];
  }
#pragma unroll
  for (int i = 0; i < 4; i++) qt[i] = state[(RG_SRB_ROW_QUAT + i) * sB + b];
  const double stance = state[(RG_SRB_ROW_STANCE + leg) * sB + b];
  const double steps = state[RG_SRB_ROW_STEPS * sB + b];
  const bool running = state[RG_SRB_ROW_STATUS * sB + b] == 0.0;
  const bool chosen = mask ? mask[b] != 0 : true;
#pragma unroll
  for (int l = 0; l < 4; l++) {
    const double fx = state[(RG_SRB_ROW_FOOT + 3 * l) * sB + b], fy = state[(RG_SRB_ROW_FOOT + 3 * l + 1) * sB + b];
    hs[l] = flat ? 0.0 : ground(b, fx, fy);
  }
  const double own = leg & 2 ? (leg & 1 ? hs[3] : hs[2]) : (leg & 1 ? hs[1] : hs[0]);
  foot[2] = own;
  p[2] = p[2] + ((hs[0] + hs[1]) + (hs[2] + hs[3])) * 0.25;
  const bool store = in_batch && running && chosen;
  if (store) {
    state[(RG_SRB_ROW_FOOT + 3 * leg + 2) * sB + b] = foot[2];
    if (leg == 0) state[(RG_SRB_ROW_P + 2) * sB + b] = p[2];
  }
  write_obs(kc, c, o, state, b, leg, store, p, qt, v, w, foot, q, stance, steps, RG_SRB_RESET_IK_PASSES);
}

// out[k] = h(x_k, y_k; robot_k)
__global__ void __launch_bounds__(kBlock) rg_srb_terrain_height_kernel(rg_srb_ground g, int B, const double *__restrict__ xy,
                                                                        const int *__restrict__ robot, int n, double *__restrict__ out) {
  const int k = blockIdx.x * kBlock + threadIdx.x;
  if (k >= n) return;   // no cross-lane operation in this kernel
  if (g.kind == RG_SRB_TERRAIN_FLAT) { out[k] = 0.0; return; }
  int b = robot ? robot[k] : k;
  b = b < 0 ? 0 : (b >= B ? B - 1 : b);   // the key row has B entries: an index outside it reads the nearest one, never past it
  out[k] = Ground{g}(b, xy[k], xy[(size_t)n + k]);
}

bool refuse(char *msg, int n, const char *text) {
  if (msg && n > 0) snprintf(msg, (size_t)n, "%s", text);
  return false;
}

bool terrain_valid(const rg_srb_terrain *t, char *msg, int n) {
  char buf[200];
  if (!t) return refuse(msg, n, "terrain: null");
  std::string err;
  if (!check_abi("terrain.", t->abi_version, RG_SRB_ABI_VERSION, err)) return refuse(msg, n, err.c_str());
  if (t->kind != RG_SRB_TERRAIN_FLAT && t->kind != RG_SRB_TERRAIN_RANDOM && t->kind != RG_SRB_TERRAIN_GRID) {
    snprintf(buf, sizeof(buf), "terrain.kind: %d is not 0 (flat), 1 (random) or 2 (grid)", t->kind);
    return refuse(msg, n, buf);
  }
  for (int i = 0; i < 4; i++)
    if (t->reserved[i] != 0) { snprintf(buf, sizeof(buf), "terrain.reserved[%d]: must be 0", i); return refuse(msg, n, buf); }
  struct F { const char *name; double v; };
  const F fields[] = {{"cell", t->cell}, {"amplitude", t->amplitude}, {"x0", t->x0}, {"y0", t->y0}};
  for (const F &f : fields)
    if (!std::isfinite(f.v)) { snprintf(buf, sizeof(buf), "terrain.%s: %g is not finite", f.name, f.v); return refuse(msg, n, buf); }
  const bool random = t->kind == RG_SRB_TERRAIN_RANDOM, grid = t->kind == RG_SRB_TERRAIN_GRID;
  if (random || grid) {
    if (!(t->cell > 0)) { snprintf(buf, sizeof(buf), "terrain.cell: %g must be > 0", t->cell); return refuse(msg, n, buf); }
  } else if (t->cell != 0) return refuse(msg, n, "terrain.cell: must be 0 for the flat kind");
  if (random) {
    if (!(t->amplitude >= 0)) { snprintf(buf, sizeof(buf), "terrain.amplitude: %g must be >= 0", t->amplitude); return refuse(msg, n, buf); }
  } else {
    if (t->amplitude != 0) return refuse(msg, n, "terrain.amplitude: must be 0 unless the kind is random");
    if (t->seed != 0) return refuse(msg, n, "terrain.seed: must be 0 unless the kind is random");
    if (t->key) return refuse(msg, n, "terrain.key: must be NULL unless the kind is random");
  }
  if (grid) {
    if (!t->heights) return refuse(msg, n, "terrain.heights: NULL for the grid kind");
    if (t->rows < 2 || t->rows > RG_SRB_TERRAIN_MAX_DIM) {
      snprintf(buf, sizeof(buf), "terrain.rows: %d outside [2, %d]", t->rows, RG_SRB_TERRAIN_MAX_DIM);
      return refuse(msg, n, buf);
    }
    if (t->cols < 2 || t->cols > RG_SRB_TERRAIN_MAX_DIM) {
      snprintf(buf, sizeof(buf), "terrain.cols: %d outside [2, %d]", t->cols, RG_SRB_TERRAIN_MAX_DIM);
      return refuse(msg, n, buf);
    }
  } else {
    if (t->heights) return refuse(msg, n, "terrain.heights: must be NULL unless the kind is grid");
    if (t->rows != 0) return refuse(msg, n, "terrain.rows: must be 0 unless the kind is grid");
    if (t->cols != 0) return refuse(msg, n, "terrain.cols: must be 0 unless the kind is grid");
    if (t->x0 != 0) return refuse(msg, n, "terrain.x0: must be 0 unless the kind is grid");
    if (t->y0 != 0) return refuse(msg, n, "terrain.y0: must be 0 unless the kind is grid");
  }
  return true;
}

}  // namespace

int rg_srb_terrain_step_launch(rg_srb_handle *h, double *state, const float *grf, const float *foot_target, const int32_t *desired_state,
                               const double *ext, const rg_srb_obs_ptrs *obs, hipStream_t s) {
  const unsigned lanes = 4u * (unsigned)h->B;
  hipLaunchKernelGGL(rg_srb_terrain_step_kernel, dim3((lanes + kBlock - 1) / kBlock), dim3(kBlock), 0, s, h->dcfg, h->c, h->ground, h->body,
                     state, grf, foot_target, desired_state, ext, to_obs(obs));
  return launch_status(h, "rg_srb_terrain_step_kernel launch");
}

int rg_srb_terrain_settle_launch(rg_srb_handle *h, double *state, const int32_t *mask, const rg_srb_obs_ptrs *obs, hipStream_t s) {
  const unsigned lanes = 4u * (unsigned)h->B;
  hipLaunchKernelGGL(rg_srb_terrain_settle_kernel, dim3((lanes + kBlock - 1) / kBlock), dim3(kBlock), 0, s, h->dcfg, h->c, h->ground,
                     h->ground.kind == RG_SRB_TERRAIN_FLAT ? 1 : 0, state, mask, to_obs(obs));
  return launch_status(h, "rg_srb_terrain_settle_kernel launch");
}

extern "C" {

int32_t rg_srb_terrain_size(void) { return (int32_t)sizeof(rg_srb_terrain); }

int rg_srb_terrain_check(const rg_srb_terrain *t, char *msg, int32_t n) {
  if (msg && n > 0) msg[0] = 0;
  return terrain_valid(t, msg, n) ? RG_SRB_OK : RG_SRB_ERR_INVALID;
}

int rg_srb_set_terrain(rg_srb_handle *h, const rg_srb_terrain *t) {
  if (!h) { rg_srb_thread_error("set_terrain: null handle"); return RG_SRB_ERR_INVALID; }
  if (!t || t->kind == RG_SRB_TERRAIN_FLAT) {
    char msg[200];
    if (t && !terrain_valid(t, msg, sizeof(msg))) { h->err = std::string("set_terrain: ") + msg; return RG_SRB_ERR_INVALID; }
    h->ground = rg_srb_ground();
    return RG_SRB_OK;
  }
  char msg[200];
  if (!terrain_valid(t, msg, sizeof(msg))) { h->err = std::string("set_terrain: ") + msg; return RG_SRB_ERR_INVALID; }
  if (!h->reset_mask) {
    DeviceScope dev(h->device);
    if (dev.err != hipSuccess) return hip_fail(h, "hipSetDevice failed", dev.err);
    const hipError_t e = hipMalloc((void **)&h->reset_mask, (size_t)h->B * sizeof(int32_t));
    if (e != hipSuccess) { h->reset_mask = nullptr; h->err = std::string("set_terrain: hipMalloc failed: ") + hipGetErrorString(e); return RG_SRB_ERR_ALLOC; }
  }
  rg_srb_ground g;
  g.kind = t->kind; g.rows = t->rows; g.cols = t->cols;
  g.cell = t->cell; g.amplitude = t->amplitude; g.x0 = t->x0; g.y0 = t->y0;
  g.seed = (unsigned long long)t->seed;
  g.key = (const long long *)t->key; g.heights = t->heights;
  h->ground = g;
  return RG_SRB_OK;
}

int rg_srb_ground_height(rg_srb_handle *h, const double *xy, const int32_t *robot, int32_t n, double *out, void *stream) {
  if (!h) { rg_srb_thread_error("ground_height: null handle"); return RG_SRB_ERR_INVALID; }
  if (!xy || !out) { h->err = "ground_height: null xy or out"; return RG_SRB_ERR_INVALID; }
  if (n < 1 || n > RG_SRB_MAX_BATCH) { h->err = "ground_height: n outside [1, RG_SRB_MAX_BATCH]"; return RG_SRB_ERR_INVALID; }
  if (!robot && n > h->B) { h->err = "ground_height: without a robot list entry k is robot k, so n must not exceed the batch"; return RG_SRB_ERR_INVALID; }
  DeviceScope dev(h->device);
  if (dev.err != hipSuccess) return hip_fail(h, "hipSetDevice failed", dev.err);
  hipLaunchKernelGGL(rg_srb_terrain_height_kernel, dim3(((unsigned)n + kBlock - 1) / kBlock), dim3(kBlock), 0, (hipStream_t)stream, h->ground,
                     h->B, xy, robot, n, out);
  return launch_status(h, "rg_srb_terrain_height_kernel launch");
}

int rg_srb_settle(rg_srb_handle *h, double *state, const int32_t *mask, const rg_srb_obs_ptrs *obs, void *stream) {
  if (!h) { rg_srb_thread_error("settle: null handle"); return RG_SRB_ERR_INVALID; }
  if (!state || !obs_ok(obs)) { h->err = "settle: null state or observation pointer"; return RG_SRB_ERR_INVALID; }
  DeviceScope dev(h->device);
  if (dev.err != hipSuccess) return hip_fail(h, "hipSetDevice failed", dev.err);
  return rg_srb_terrain_settle_launch(h, state, mask, obs, (hipStream_t)stream);
}

}  // extern "C"

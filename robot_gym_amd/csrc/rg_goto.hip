// rg_goto.hip -- the batched go-to-target task of include/rg_goto.h.  Its own translation unit of librg_mpc.so.
//
// Layout of the tick kernel: one 64-lane wave per robot, one wave per workgroup, because a robot's work is a scan over its
// (at most n_max) path points and every branch of the tick is then uniform over the workgroup.  The lanes read x and y in
// coalesced 64-point chunks; one pass keeps the running (distance, lowest index) to pos and to prev_pos and tests
// the window, compacting the visible points in path order into LDS with a ballot and a prefix count.  Each lane then holds
// visible points `lane` and `lane + 64` in registers; the greedy chain is one wave arg-min (an xor butterfly on
// (distance, index), so every lane ends with the same winner) per link, the chain and its cumulative length go to LDS,
// lanes 0 .. num_cam_pts-1 each resample one point, and lane 0 stores the scalars.  The reward and termination values
// are uniform over the wave and computed by every lane.  No global read-modify-write, no scratch.
// LDS: 5 arrays of RG_GOTO_MAX_VISIBLE doubles = 5120 bytes per workgroup.
//
// Parity: tests/goto_model.py restates this file operation for operation in float64 numpy.  Contraction is off.  What
// remains different: the device's atan2 / sincos / sqrt / division against libm's.
#include <hip/hip_runtime.h>
#include <math.h>
#include <climits>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>
#include "../../include/rg_goto.h"
#include "../../include/rg_srb.h"
#include "rg_host.h"

#pragma clang fp contract(off)

namespace {

constexpr int kPreBlock = 256;
constexpr int kStageRows = 5;   // set_path staging [kStageRows][n]: robot, npts, length, target x, target y

// GotoCfg, Paths, wave_argmin, yaw_of, goto_observe (steps 1 and 2 of the tick) and the configuration checks: shared with
// rg_episode.hip
#include "rg_goto_dev.inc"

__global__ void __launch_bounds__(kWave) rg_goto_post_kernel(GotoCfg c, int observe_only, double *__restrict__ task,
                                                            const double *__restrict__ sim, Paths P, float *__restrict__ obs,
                                                            float *__restrict__ reward, int *__restrict__ done_out) {
  __shared__ double vx[kMaxVis], vy[kMaxVis];                 // visible points, robot frame, path order
  __shared__ double cx[kMaxVis], cy[kMaxVis], cs[kMaxVis];    // the chain and its cumulative length
  const int b = blockIdx.x, lane = threadIdx.x;
  const size_t sB = (size_t)c.B;
  int n = (int)P.hdr[b];
  n = n > c.n_max ? c.n_max : n;
  const bool frozen = task[RG_GOTO_ROW_DONE * sB + b] != 0.0 || n < 2;
  if (frozen) {   // uniform over the workgroup
    if (lane < 2 * c.ncp) obs[lane * sB + b] = (float)task[(RG_GOTO_ROW_OBS + lane) * sB + b];
    if (lane == 0 && !observe_only) { reward[b] = 0.0f; done_out[b] = 1; }
    return;
  }
  // 1. pose
  const double ox = task[(RG_GOTO_ROW_POS + 0) * sB + b], oy = task[(RG_GOTO_ROW_POS + 1) * sB + b], oyaw = task[(RG_GOTO_ROW_POS + 2) * sB + b];
  double px = sim[(RG_SRB_ROW_P + 0) * sB + b], py = sim[(RG_SRB_ROW_P + 1) * sB + b], yaw = yaw_of(sim, sB, b);
  const bool bad = !(isfinite(px) && isfinite(py) && isfinite(yaw));
  if (bad) { px = ox; py = oy; yaw = oyaw; }
  const bool fallen = bad || sim[RG_SRB_ROW_STATUS * sB + b] != 0.0;
  // 2. observation: window, visible points, chain, interpolation; the nearest path point to pos and to prev_pos
  const double *X = P.x + (size_t)b * c.n_max, *Y = P.y + (size_t)b * c.n_max, *S = P.s + (size_t)b * c.n_max;
  const int *F = P.fsx + (size_t)b * c.n_max;
  double bd;
  int bi, bpi;
  goto_observe(c, b, lane, n, task, X, Y, px, py, yaw, ox, oy, oyaw, obs, vx, vy, cx, cy, cs, bd, bi, bpi);
  if (observe_only) return;
  // 3. reward (uniform over the wave)
  const int last = n - 1;
  bi = bi > last ? 0 : bi;       // INT_MAX only if no distance compared (a path slab overwritten with NaN): stay in bounds
  bpi = bpi > last ? 0 : bpi;
  int i1 = F[bpi], i2 = F[bi];
  i1 = i1 < 0 ? 0 : (i1 > last ? last : i1);
  i2 = i2 < 0 ? 0 : (i2 > last ? last : i2);
  const double track_err = bd;
  const double err_norm = track_err * c.inv_max_err;
  double dl = 0.0;
  if (i1 != i2) {
    const int first = i1 < i2 ? i1 : i2, second = i1 < i2 ? i2 : i1;
    const double len1 = S[second] - S[first];
    const double gx = X[second] - X[first], gy = Y[second] - Y[first];
    const double len2 = S[first] + sqrt(gx * gx + gy * gy) + (S[last] - S[second]);
    if (len1 < len2) dl = i1 < i2 ? len1 : -len1;
    else dl = i1 < i2 ? -len2 : len2;
  }
  double pot = task[RG_GOTO_ROW_POT * sB + b] + dl;
  double progress = task[RG_GOTO_ROW_PROGRESS * sB + b];
  int nci = (int)task[RG_GOTO_ROW_NEXT_CP * sB + b];
  bool path_done = task[RG_GOTO_ROW_PATH_DONE * sB + b] != 0.0;
  const double length = P.hdr[sB + b];
  double r = 0.0;
  if (pot - progress < c.prog_window) {
    int k = 0;
    if (!path_done) {
      if (pot > progress) progress = pot;
      const double per = length / (double)c.ncheck;
      while (k < c.ncheck && progress >= (double)(nci + 1) * per) {
        nci++;
        k++;
        if (nci >= c.ncheck - 1) { path_done = true; break; }
      }
    }
    const double u = 1.0 - err_norm;
    r = r + (double)k * c.cp_reward * (u * u);
  }
  r = r - c.penalty;
  const bool off_progress = fabs(pot - progress) > c.prog_limit, off_track = track_err > c.max_err;
  if (off_progress || off_track) r = RG_GOTO_LIMIT_REWARD;
  // 4. termination
  const double tgx = px - P.hdr[2 * sB + b], tgy = py - P.hdr[3 * sB + b];
  const bool on_target = sqrt(tgx * tgx + tgy * tgy) <= c.radius;
  int reason = RG_GOTO_REASON_NONE;
  if (fallen) reason = RG_GOTO_REASON_FALLEN;
  else if (path_done) reason = RG_GOTO_REASON_PATH_DONE;
  else if (on_target) reason = RG_GOTO_REASON_ON_TARGET;
  else if (off_progress) reason = RG_GOTO_REASON_PROGRESS;
  else if (off_track) reason = RG_GOTO_REASON_TRACK;
  else if (sim[RG_SRB_ROW_STEPS * sB + b] > c.max_steps) reason = RG_GOTO_REASON_TIME;
  if (lane == 0) {
    task[RG_GOTO_ROW_POT * sB + b] = pot;
    task[RG_GOTO_ROW_PROGRESS * sB + b] = progress;
    task[RG_GOTO_ROW_NEXT_CP * sB + b] = (double)nci;
    task[RG_GOTO_ROW_PATH_DONE * sB + b] = path_done ? 1.0 : 0.0;
    task[RG_GOTO_ROW_ENV_STEPS * sB + b] = task[RG_GOTO_ROW_ENV_STEPS * sB + b] + 1.0;
    task[RG_GOTO_ROW_DONE * sB + b] = reason ? 1.0 : 0.0;
    task[RG_GOTO_ROW_REASON * sB + b] = (double)reason;
    task[RG_GOTO_ROW_TRACK_ERR * sB + b] = track_err;
    reward[b] = (float)r;
    done_out[b] = reason ? 1 : 0;
  }
}

__global__ void __launch_bounds__(kPreBlock) rg_goto_pre_kernel(GotoCfg c, const double *__restrict__ task, const double *__restrict__ sim,
                                                                const double *__restrict__ hdr, const float *__restrict__ action,
                                                                float *__restrict__ cmd) {
  const int b = blockIdx.x * kPreBlock + threadIdx.x;
  if (b >= c.B) return;   // no cross-lane operation in this kernel
  const size_t sB = (size_t)c.B;
  double a[2] = {(double)action[2 * (size_t)b], (double)action[2 * (size_t)b + 1]};
#pragma unroll
  for (int i = 0; i < 2; i++) {
    if (!(a[i] == a[i])) a[i] = 0.0;
    a[i] = a[i] < c.lo[i] ? c.lo[i] : (a[i] > c.hi[i] ? c.hi[i] : a[i]);
  }
  const double tx = sim[(RG_SRB_ROW_P + 0) * sB + b] - hdr[2 * sB + b], ty = sim[(RG_SRB_ROW_P + 1) * sB + b] - hdr[3 * sB + b];
  const bool stand = task[RG_GOTO_ROW_DONE * sB + b] != 0.0 || hdr[b] < 2.0 || sqrt(tx * tx + ty * ty) <= c.radius;
  if (stand) { a[0] = 0.0; a[1] = 0.0; }
  cmd[b] = (float)a[0] + c.off[0];
  cmd[sB + b] = 0.0f + c.off[1];
  cmd[2 * sB + b] = (float)a[1] + c.off[2];
}

// set_path: header columns from the staging rows, task state columns zeroed.  One thread per entry.
__global__ void __launch_bounds__(kPreBlock) rg_goto_set_kernel(int B, int n, const double *__restrict__ st, double *__restrict__ hdr,
                                                                double *__restrict__ task) {
  const int k = blockIdx.x * kPreBlock + threadIdx.x;
  if (k >= n) return;
  const size_t sB = (size_t)B, sn = (size_t)n;
  const int b = (int)st[k];
  for (int r = 0; r < RG_GOTO_HDR_ROWS; r++) hdr[r * sB + b] = st[(1 + r) * sn + k];
  for (int r = 0; r < RG_GOTO_STATE_ROWS; r++) task[r * sB + b] = 0.0;
}

thread_local std::string g_create_err;

}  // namespace

struct rg_goto_handle {
  GotoCfg c{};
  rg_goto_config cfg{};
  int B = 0, device = 0;
  double *stage = nullptr;   // [kStageRows][B]
  std::vector<double> stage_host;
  std::string err;
};

namespace {

int hip_fail(rg_goto_handle *h, const char *what, hipError_t e) { return hip_fail(h, RG_GOTO_ERR_HIP, what, e); }
int no_device(rg_goto_handle *h) { return no_device(h, RG_GOTO_ERR_NO_DEVICE, "RG_GOTO"); }
int launch_status(rg_goto_handle *h, const char *what) { return launch_status(h, RG_GOTO_ERR_HIP, what); }
int null_arg(rg_goto_handle *h, const char *call, const char *name) { return null_arg(h, RG_GOTO_ERR_INVALID, call, name); }

int post(rg_goto_handle *h, const char *who, int observe_only, double *task_state, const double *sim_state, const rg_goto_path_ptrs *paths,
         float *obs, float *reward, int32_t *done, void *stream) {
  if (!h) { g_create_err = std::string(who) + ": null handle"; return RG_GOTO_ERR_INVALID; }
  RG_NEED(who, task_state, "task_state");
  RG_NEED(who, sim_state, "sim_state");
  RG_NEED(who, paths_ok(paths), "paths pointer");
  RG_NEED(who, obs, "obs");
  if (!observe_only) RG_NEED(who, reward && done, "reward or done");
  if (h->device < 0) return no_device(h);
  DeviceScope dev(h->device);
  if (dev.err != hipSuccess) return hip_fail(h, "hipSetDevice failed", dev.err);
  hipLaunchKernelGGL(rg_goto_post_kernel, dim3((unsigned)h->B), dim3(kWave), 0, (hipStream_t)stream, h->c, observe_only, task_state, sim_state,
                     to_paths(paths), obs, reward, done);
  return launch_status(h, "rg_goto_post_kernel launch");
}

}  // namespace

extern "C" {

int32_t rg_goto_abi_version(void) { return RG_GOTO_ABI_VERSION; }
int32_t rg_goto_config_size(void) { return (int32_t)sizeof(rg_goto_config); }
int32_t rg_goto_state_rows(void) { return RG_GOTO_STATE_ROWS; }
const char *rg_goto_last_error(const rg_goto_handle *h) { return h ? h->err.c_str() : g_create_err.c_str(); }

int rg_goto_create(const rg_goto_config *cfg, int32_t batch, int32_t device, rg_goto_handle **out) {
  if (!cfg || !out) { g_create_err = "create: null config or out"; return RG_GOTO_ERR_INVALID; }
  *out = nullptr;
  std::string err;
  if (!goto_validate(cfg, batch, err)) { g_create_err = err; return RG_GOTO_ERR_INVALID; }
  rg_goto_handle *h = new rg_goto_handle();
  h->B = batch;
  h->device = device;
  h->cfg = *cfg;
  goto_fill_cfg(cfg, batch, h->c);
  h->stage_host.resize((size_t)kStageRows * batch);
  if (device == RG_GOTO_DEVICE_NONE) {   // a host-only handle: the configuration, for argument checks on any machine
    *out = h;
    return RG_GOTO_OK;
  }
  std::optional<DeviceScope> dev;
  if (const int rc = enter_device(device, &dev, RG_GOTO_ERR_NO_DEVICE, RG_GOTO_ERR_INVALID, RG_GOTO_ERR_HIP, g_create_err)) { delete h; return rc; }
  const hipError_t e = hipMalloc((void **)&h->stage, (size_t)kStageRows * batch * sizeof(double));
  if (e != hipSuccess) {
    g_create_err = std::string("hipMalloc failed: ") + hipGetErrorString(e);
    rg_goto_destroy(h);
    return RG_GOTO_ERR_ALLOC;
  }
  *out = h;
  return RG_GOTO_OK;
}

void rg_goto_destroy(rg_goto_handle *h) {
  if (!h) return;
  if (h->device >= 0) {
    DeviceScope dev(h->device);
    if (h->stage) (void)hipFree(h->stage);
  }
  delete h;
}

int rg_goto_set_path(rg_goto_handle *h, const int32_t *idx_host, int32_t n, const int32_t *npts, const double *length,
                     const double *target, const double *x, const double *y, const double *s, const int32_t *first_same_x,
                     const rg_goto_path_ptrs *paths, double *task_state, void *stream) {
  if (!h) { g_create_err = "set_path: null handle"; return RG_GOTO_ERR_INVALID; }
  RG_NEED("set_path", npts && length && target && x && y && s && first_same_x, "host array");
  RG_NEED("set_path", paths_ok(paths), "paths pointer");
  RG_NEED("set_path", task_state, "task_state");
  const int B = h->B, n_max = h->c.n_max;
  if (idx_host ? (n < 1 || n > B) : n != B) { h->err = "set_path: n must be the batch without an index list, 1..batch with one"; return RG_GOTO_ERR_INVALID; }
  const size_t sn = (size_t)n;
  char msg[200];
  std::vector<char> taken(idx_host ? (size_t)B : 0, 0);
  double *st = h->stage_host.data();
  for (int k = 0; k < n; k++) {
    const int b = idx_host ? idx_host[k] : k;
    auto bad = [&](const char *what) {
      snprintf(msg, sizeof(msg), "set_path: entry %d (robot %d): %s", k, b, what);
      h->err = msg;
      return RG_GOTO_ERR_INVALID;
    };
    if (b < 0 || b >= B) return bad("robot out of range");
    if (idx_host) {
      if (taken[b]) return bad("robot given twice");
      taken[b] = 1;
    }
    if (npts[k] > n_max) { snprintf(msg, sizeof(msg), "set_path: entry %d (robot %d): npts %d above n_max %d", k, b, npts[k], n_max); h->err = msg; return RG_GOTO_ERR_INVALID; }
    if (npts[k] < 2) { snprintf(msg, sizeof(msg), "set_path: entry %d (robot %d): npts %d below 2", k, b, npts[k]); h->err = msg; return RG_GOTO_ERR_INVALID; }
    if (!(length[k] > 0 && length[k] <= 1e300)) return bad("length must be positive and finite");
    if (!(fabs(target[k]) <= 1e300 && fabs(target[sn + k]) <= 1e300)) return bad("target must be finite");
    const size_t row = (size_t)k * n_max;
    for (int i = 0; i < npts[k]; i++) {
      if (!(fabs(x[row + i]) <= 1e300 && fabs(y[row + i]) <= 1e300 && fabs(s[row + i]) <= 1e300)) return bad("x, y and s must be finite");
      if (first_same_x[row + i] < 0 || first_same_x[row + i] > i) return bad("first_same_x[i] outside [0, i]");
    }
    st[k] = (double)b; st[sn + k] = (double)npts[k]; st[2 * sn + k] = length[k]; st[3 * sn + k] = target[k]; st[4 * sn + k] = target[sn + k];
  }
  if (h->device < 0) return no_device(h);
  DeviceScope dev(h->device);
  if (dev.err != hipSuccess) return hip_fail(h, "hipSetDevice failed", dev.err);
  hipStream_t q = (hipStream_t)stream;
  hipError_t e = hipMemcpyAsync(h->stage, st, kStageRows * sn * sizeof(double), hipMemcpyHostToDevice, q);
  const size_t rd = (size_t)n_max * sizeof(double), ri = (size_t)n_max * sizeof(int32_t);
  if (!idx_host) {   // the whole slab, one copy per array
    if (e == hipSuccess) e = hipMemcpyAsync(paths->x, x, sn * rd, hipMemcpyHostToDevice, q);
    if (e == hipSuccess) e = hipMemcpyAsync(paths->y, y, sn * rd, hipMemcpyHostToDevice, q);
    if (e == hipSuccess) e = hipMemcpyAsync(paths->s, s, sn * rd, hipMemcpyHostToDevice, q);
    if (e == hipSuccess) e = hipMemcpyAsync(paths->first_same_x, first_same_x, sn * ri, hipMemcpyHostToDevice, q);
  } else {
    for (int k = 0; k < n && e == hipSuccess; k++) {
      const size_t src = (size_t)k * n_max, dst = (size_t)idx_host[k] * n_max;
      e = hipMemcpyAsync(paths->x + dst, x + src, rd, hipMemcpyHostToDevice, q);
      if (e == hipSuccess) e = hipMemcpyAsync(paths->y + dst, y + src, rd, hipMemcpyHostToDevice, q);
      if (e == hipSuccess) e = hipMemcpyAsync(paths->s + dst, s + src, rd, hipMemcpyHostToDevice, q);
      if (e == hipSuccess) e = hipMemcpyAsync(paths->first_same_x + dst, first_same_x + src, ri, hipMemcpyHostToDevice, q);
    }
  }
  if (e != hipSuccess) return hip_fail(h, "set_path copy", e);
  hipLaunchKernelGGL(rg_goto_set_kernel, dim3(((unsigned)n + kPreBlock - 1) / kPreBlock), dim3(kPreBlock), 0, q, B, n, h->stage, paths->hdr, task_state);
  const int rc = launch_status(h, "rg_goto_set_kernel launch");
  if (rc) return rc;
  e = hipStreamSynchronize(q);   // the staging buffer and the caller's host arrays are free after this
  return e != hipSuccess ? hip_fail(h, "set_path", e) : RG_GOTO_OK;
}

int rg_goto_pre_step(rg_goto_handle *h, const double *task_state, const double *sim_state, const rg_goto_path_ptrs *paths,
                     const float *action, float *cmd_out, void *stream) {
  if (!h) { g_create_err = "pre_step: null handle"; return RG_GOTO_ERR_INVALID; }
  RG_NEED("pre_step", task_state, "task_state");
  RG_NEED("pre_step", sim_state, "sim_state");
  RG_NEED("pre_step", paths_ok(paths), "paths pointer");
  RG_NEED("pre_step", action, "action");
  RG_NEED("pre_step", cmd_out, "cmd_out");
  if (h->device < 0) return no_device(h);
  DeviceScope dev(h->device);
  if (dev.err != hipSuccess) return hip_fail(h, "hipSetDevice failed", dev.err);
  hipLaunchKernelGGL(rg_goto_pre_kernel, dim3(((unsigned)h->B + kPreBlock - 1) / kPreBlock), dim3(kPreBlock), 0, (hipStream_t)stream, h->c,
                     task_state, sim_state, paths->hdr, action, cmd_out);
  return launch_status(h, "rg_goto_pre_kernel launch");
}

int rg_goto_post_step(rg_goto_handle *h, double *task_state, const double *sim_state, const rg_goto_path_ptrs *paths,
                      float *obs, float *reward, int32_t *done, void *stream) {
  return post(h, "post_step", 0, task_state, sim_state, paths, obs, reward, done, stream);
}

int rg_goto_observe(rg_goto_handle *h, double *task_state, const double *sim_state, const rg_goto_path_ptrs *paths, float *obs, void *stream) {
  return post(h, "observe", 1, task_state, sim_state, paths, obs, nullptr, nullptr, stream);
}

}  // extern "C"

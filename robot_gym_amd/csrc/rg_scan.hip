// rg_scan.hip -- the terrain height scan of include/rg_scan.h: under a fixed grid of points in the robot's yaw frame, the
// height of the body above the simulator's ground (rg_srb_ground.inc, shared with rg_srb_terrain.hip and
// rg_srb_contact.hip), written into rows of a component-major float32 observation.  Its own translation unit of
// librg_mpc.so, so that the simulator's units keep reporting exactly their kernels.
//
// Layout: lane = robot, float64, no LDS, no cross-lane operation.  Consecutive lanes are consecutive robots, so the seven
// state-row loads and every row store coalesce.  A lane loads its pose once, forms the heading once and walks the points
// [blockIdx.y * per, blockIdx.y * per + per) of the grid; `per` is chosen at create from the configuration and the batch
// (enough waves to cover the device at a small batch, few repeats of the heading at a large one) and no output depends on
// it.  Lanes past the batch compute on the last robot and are guarded at their stores; a robot outside the mask leaves
// after the mask load, so a wave with no robot to scan costs a load and an exit.
//
// Parity: tests/scan_model.py restates the arithmetic of rg_scan.h in float64 numpy, bit for bit.  Floating-point
// contraction is off for the whole file.
#include <hip/hip_runtime.h>
#include <math.h>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>
#include "../../include/rg_scan.h"
#include "rg_host.h"

#pragma clang fp contract(off)

#include "rg_mpc_dev.h"

namespace {

#include "rg_srb_dev.inc"

}  // namespace

#include "rg_srb_handle.h"

struct rg_scan_handle {
  rg_scan_config cfg;
  int B = 0, device = 0;
  int per = 1;            // points a lane walks
  rg_srb_ground ground;   // rg_scan_set_terrain; kind 0: the plane
  std::string err;
};

namespace {

constexpr int kBlock = 64;           // one wave: 64 robots
constexpr int kTargetWaves = 2048;   // the points are split until a launch has about this many waves (two per SIMD of 256 CUs)

// kCoordBound, the hash chain and Ground, h(x, y; robot) of rg_srb.h
#include "rg_srb_ground.inc"

struct ScanCfg {
  int B, nx, ny, per;
  double x_first, dx, y_first, dy, z_offset, clip, scale;
};

__global__ void __launch_bounds__(kBlock) rg_scan_observe_kernel(ScanCfg c, rg_srb_ground g, const double *__restrict__ state,
                                                                  const int *__restrict__ mask, float *__restrict__ out,
                                                                  float *__restrict__ prev) {
  const int t = blockIdx.x * kBlock + threadIdx.x;
  const bool in_batch = t < c.B;
  const int b = in_batch ? t : c.B - 1;   // lanes past the batch compute on the last robot and store nothing
  const size_t sB = (size_t)c.B;
  const bool store = in_batch && (mask ? mask[b] != 0 : true);
  if (!store) return;   // no cross-lane operation in this kernel
  const double px = state[(RG_SRB_ROW_P + 0) * sB + b], py = state[(RG_SRB_ROW_P + 1) * sB + b], pz = state[(RG_SRB_ROW_P + 2) * sB + b];
  const double qx = state[(RG_SRB_ROW_QUAT + 0) * sB + b], qy = state[(RG_SRB_ROW_QUAT + 1) * sB + b];
  const double qz = state[(RG_SRB_ROW_QUAT + 2) * sB + b], qw = state[(RG_SRB_ROW_QUAT + 3) * sB + b];
  // the heading: the first column of R, normalised
  const double c0 = 1 - 2 * (qy * qy + qz * qz), s0 = 2 * (qx * qy + qz * qw);
  const double n = sqrt(c0 * c0 + s0 * s0);
  const bool turned = n > 0;   // false for a NaN
  const double ch = turned ? c0 / n : 1.0, sh = turned ? s0 / n : 0.0;
  const double base = pz - c.z_offset;
  // The prefix mix_word(seed, key) of the random ground is the robot's, not the point's: mix_word(h, w) reads h ^ w only,
  // so the robot's key folded into the seed, with no key row, is the same chain -- of loop-invariant registers, which the
  // compiler computes once, where a load of key[b] between the stores below would stay in the loop.
  Ground ground{g};
  if (g.kind == RG_SRB_TERRAIN_RANDOM && g.key) {
    ground.g.seed = g.seed ^ (unsigned long long)g.key[b];
    ground.g.key = nullptr;
  }
  const bool flat = g.kind == RG_SRB_TERRAIN_FLAT;
  const int N = c.nx * c.ny;
  const int k0 = (int)blockIdx.y * c.per;
  const int k1 = k0 + c.per < N ? k0 + c.per : N;
  int a = k0 / c.ny, cc = k0 - a * c.ny;
  for (int k = k0; k < k1; k++) {
    const double fx = c.x_first + (double)a * c.dx, fy = c.y_first + (double)cc * c.dy;
    const double X = px + (ch * fx - sh * fy), Y = py + (sh * fx + ch * fy);
    const double h = flat ? 0.0 : ground(b, X, Y);
    double d = base - h;
    if (c.clip > 0) d = fmin(fmax(d, -c.clip), c.clip);   // a NaN becomes the lower bound
    const size_t at = (size_t)k * sB + b;
    if (prev) prev[at] = out[at];
    out[at] = (float)(d * c.scale);
    if (++cc == c.ny) { cc = 0; a++; }
  }
}

thread_local std::string g_create_err;

bool validate(const rg_scan_config *cfg, std::string &err) {
  if (!check_abi("config.", cfg->abi_version, RG_SCAN_ABI_VERSION, err) || !check_reserved("config.", "reserved0", cfg->reserved0, err) ||
      !check_reserved("config.", "reserved1", cfg->reserved1, err) || !check_reserved("config.", "reserved2", cfg->reserved2, err))
    return false;
  const IntField ints[] = {{"nx", cfg->nx, 1, RG_SCAN_MAX_POINTS}, {"ny", cfg->ny, 1, RG_SCAN_MAX_POINTS}};
  if (cfg->nx >= 1 && cfg->ny >= 1 && (long long)cfg->nx * cfg->ny > RG_SCAN_MAX_POINTS) {
    char msg[200];
    snprintf(msg, sizeof(msg), "config.nx * ny: %lld points, at most %d (RG_SCAN_MAX_POINTS)", (long long)cfg->nx * cfg->ny, RG_SCAN_MAX_POINTS);
    err = msg;
    return false;
  }
  const RealField reals[] = {{"x_first", &cfg->x_first, 1, kFinite}, {"dx", &cfg->dx, 1, kFinite}, {"y_first", &cfg->y_first, 1, kFinite},
                             {"dy", &cfg->dy, 1, kFinite}, {"z_offset", &cfg->z_offset, 1, kFinite}, {"clip", &cfg->clip, 1, kNonNegative},
                             {"scale", &cfg->scale, 1, kFinite}};
  return check_ints("config.", ints, err) && check_reals("config.", reals, err);
}

int hip_fail(rg_scan_handle *h, const char *what, hipError_t e) { return hip_fail(h, RG_SCAN_ERR_HIP, what, e); }
int no_device(rg_scan_handle *h) { return no_device(h, RG_SCAN_ERR_NO_DEVICE, "RG_SCAN"); }
int launch_status(rg_scan_handle *h, const char *what) { return launch_status(h, RG_SCAN_ERR_HIP, what); }
int null_arg(rg_scan_handle *h, const char *call, const char *name) { return null_arg(h, RG_SCAN_ERR_INVALID, call, name); }

// points a lane walks: the fewest slices of the N points that give a launch kTargetWaves waves, as equal as they come
int points_per_lane(int N, int batch) {
  const int waves = (batch + kBlock - 1) / kBlock;
  int slices = (kTargetWaves + waves - 1) / waves;
  slices = slices < 1 ? 1 : (slices > N ? N : slices);
  return (N + slices - 1) / slices;
}

}  // namespace

extern "C" {

int32_t rg_scan_abi_version(void) { return RG_SCAN_ABI_VERSION; }
int32_t rg_scan_config_size(void) { return (int32_t)sizeof(rg_scan_config); }
const char *rg_scan_last_error(const rg_scan_handle *h) { return h ? h->err.c_str() : g_create_err.c_str(); }

int rg_scan_create(const rg_scan_config *cfg, int32_t batch, int32_t device, rg_scan_handle **out) {
  if (!cfg || !out) { g_create_err = "create: null config or out"; return RG_SCAN_ERR_INVALID; }
  *out = nullptr;
  std::string err;
  if (!check_batch(batch, RG_SCAN_MAX_BATCH, err) || !validate(cfg, err)) { g_create_err = err; return RG_SCAN_ERR_INVALID; }
  if (device != RG_SCAN_DEVICE_NONE)
    if (const int rc = enter_device(device, nullptr, RG_SCAN_ERR_NO_DEVICE, RG_SCAN_ERR_INVALID, RG_SCAN_ERR_HIP, g_create_err)) return rc;
  rg_scan_handle *h = new rg_scan_handle();
  h->cfg = *cfg;
  h->B = batch;
  h->device = device;
  h->per = points_per_lane(cfg->nx * cfg->ny, batch);
  *out = h;
  return RG_SCAN_OK;
}

void rg_scan_destroy(rg_scan_handle *h) { delete h; }

int rg_scan_set_terrain(rg_scan_handle *h, const rg_srb_terrain *t) {
  if (!h) { g_create_err = "set_terrain: null handle"; return RG_SCAN_ERR_INVALID; }
  rg_srb_ground g;
  if (t) {
    char msg[200];
    if (rg_srb_terrain_check(t, msg, sizeof(msg)) != RG_SRB_OK) { h->err = std::string("set_terrain: ") + msg; return RG_SCAN_ERR_INVALID; }
    if (t->kind != RG_SRB_TERRAIN_FLAT) {
      g.kind = t->kind; g.rows = t->rows; g.cols = t->cols;
      g.cell = t->cell; g.amplitude = t->amplitude; g.x0 = t->x0; g.y0 = t->y0;
      g.seed = (unsigned long long)t->seed;
      g.key = (const long long *)t->key; g.heights = t->heights;
    }
  }
  if (h->device < 0) return no_device(h);
  h->ground = g;
  return RG_SCAN_OK;
}

int rg_scan_observe(rg_scan_handle *h, const double *sim_state, const int32_t *mask, float *out, float *prev, void *stream) {
  if (!h) { g_create_err = "observe: null handle"; return RG_SCAN_ERR_INVALID; }
  RG_NEED("observe", sim_state, "sim_state");
  RG_NEED("observe", out, "out");
  if (prev == out) { h->err = "observe: prev must not alias out"; return RG_SCAN_ERR_INVALID; }
  if (h->device < 0) return no_device(h);
  DeviceScope dev(h->device);
  if (dev.err != hipSuccess) return hip_fail(h, "hipSetDevice failed", dev.err);
  const rg_scan_config &f = h->cfg;
  const ScanCfg c{h->B, f.nx, f.ny, h->per, f.x_first, f.dx, f.y_first, f.dy, f.z_offset, f.clip, f.scale};
  const unsigned N = (unsigned)(f.nx * f.ny), per = (unsigned)h->per;
  hipLaunchKernelGGL(rg_scan_observe_kernel, dim3(((unsigned)h->B + kBlock - 1) / kBlock, (N + per - 1) / per), dim3(kBlock), 0, (hipStream_t)stream,
                     c, h->ground, sim_state, mask, out, prev);
  return launch_status(h, "rg_scan_observe_kernel launch");
}

}  // extern "C"

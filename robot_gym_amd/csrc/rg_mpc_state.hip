// rg_mpc_state.hip -- state rows of the batched controller: the row layout, the host validator, and the gather / scatter
// kernels behind rg_mpc_save_state / rg_mpc_load_state / rg_mpc_copy_state (entry points in rg_mpc.hip).
//
// A row is one robot's persistent controller state as 32-bit words: a header, then the component-major fields (the device
// arrays are [k][B]), then the robot-major ones (warm start [B][RG_WARM_N], working set [B][RG_WS_MAX] bytes).  The kernels
// run one thread per (robot, word): over the component-major part consecutive lanes take consecutive robots of one word
// (the device reads coalesce), over the robot-major part consecutive words of one robot (reads and row writes coalesce).
// Everything is moved as 32-bit words with vector memory instructions; no value is interpreted except reset_time under a
// clock shift.
#include "rg_mpc_dev.h"
#include "rg_mpc_state.h"
#include "../../include/rg_mpc.h"
#include <math.h>
#include <cmath>
#include <stdio.h>
#include <string.h>

static_assert(RG_STATE_WS_MAX % 4 == 0, "robot-major fields are whole words per robot");

const RgStateField *RgStateLayout::find(const char *name) const {
  for (int i = 0; i < nfields; i++)
    if (!strcmp(f[i].name, name)) return &f[i];
  return nullptr;
}

bool rg_state_layout_build(int window, int horizon, RgStateLayout *L, std::string &err) {
  if (window < 1 || window > (1 << 20)) { err = "state layout: window must be in [1, 2^20]"; return false; }
  if (horizon != 10 && horizon != 20) { err = "state layout: horizon must be 10 or 20"; return false; }
  *L = RgStateLayout();
  L->window = window; L->horizon = horizon;
  // kind: 0 f64, 1 f32, 2 i32, 3 u8
  struct F { const char *name; int kind, count, rm; };
  const F fields[] = {
      {"reset_time", 0, 1, 0}, {"fsum", 0, 3, 0}, {"fcorr", 0, 3, 0}, {"latched", 0, 12, 0}, {"swing_q", 0, 12, 0},
      {"flags", 2, 1, 0}, {"last_desired", 2, 1, 0}, {"ring_len", 2, 1, 0}, {"ring_head", 2, 1, 0}, {"swing_valid", 2, 1, 0},
      {"cmd", 1, 3, 0}, {"warm_key", 2, 1, 0}, {"ws_cnt", 2, 1, 0}, {"hard", 2, 1, 0}, {"ncs", 2, 1, 0}, {"iters", 2, 1, 0},
      {"ring", 1, 3 * window, 0},
      {"warm_z", 1, RG_WARM_N, 1}, {"warm_y", 1, RG_WARM_N, 1}, {"ws_ids", 3, RG_STATE_WS_MAX, 1}};
  static const char *kname[] = {"f64", "f32", "i32", "u8"};
  int w = RG_STATE_HDR_WORDS;
  std::string fl;
  for (const F &x : fields) {
    RgStateField &o = L->f[L->nfields++];
    o.name = x.name; o.kind = x.kind; o.count = x.count; o.robot_major = x.rm; o.word = w;
    o.words = x.kind == 0 ? 2 * x.count : (x.kind == 3 ? x.count / 4 : x.count);
    if (!x.rm) L->words_c = w + o.words;
    w += o.words;
    char buf[96];
    snprintf(buf, sizeof(buf), "%s%s:%s:%d:%c@%d", fl.empty() ? "" : ",", x.name, kname[x.kind], x.count, x.rm ? 'r' : 'c', 4 * o.word);
    fl += buf;
  }
  L->row_words = w;
  char head[192];
  snprintf(head, sizeof(head), "rg_mpc_state v%d window=%d horizon=%d warm_n=%d ws_max=%d header_bytes=%d row_bytes=%d fields=", RG_STATE_VERSION,
           window, horizon, RG_WARM_N, RG_STATE_WS_MAX, 4 * RG_STATE_HDR_WORDS, 4 * w);
  L->desc = std::string(head) + fl;
  uint64_t hsh = 1469598103934665603ull;   // FNV-1a over the description: field list, window, horizon, RG_WARM_N, RG_WS_MAX
  for (unsigned char ch : L->desc) { hsh ^= ch; hsh *= 1099511628211ull; }
  L->hash = hsh;
  // stored working sets: constraint ids 6 * block + type of the exact bodies -- four legs at horizon 10, one or two at 20
  L->ws_id_limit = 6 * horizon * (horizon == 10 ? 4 : 2);
  if (L->ws_id_limit > 256) L->ws_id_limit = 256;
  return true;
}

bool rg_state_validate(const RgStateLayout &L, const void *rows, int n, const int32_t *dst, int batch, std::string &err) {
  if (n < 0) { err = "state: n < 0"; return false; }
  if (n > 0 && !rows) { err = "state: null rows"; return false; }
  char msg[320];
  int k = 0;
  // fmt formats one double (the offending value)
  auto bad = [&](const char *field, const char *fmt, double v) {
    char what[160];
    snprintf(what, sizeof(what), fmt, v);
    snprintf(msg, sizeof(msg), "state row %d (robot %d): %s %s", k, dst ? dst[k] : k, field, what);
    err = msg;
    return false;
  };
  if (dst) {
    for (k = 0; k < n; k++)
      if (dst[k] < 0 || dst[k] >= batch) {
        snprintf(msg, sizeof(msg), "state row %d: destination robot %d out of range [0, %d)", k, dst[k], batch);
        err = msg;
        return false;
      }
    std::string seen((size_t)batch, '\0');
    for (k = 0; k < n; k++) {
      if (seen[(size_t)dst[k]]) {
        snprintf(msg, sizeof(msg), "state row %d (robot %d): destination robot repeated", k, dst[k]);
        err = msg;
        return false;
      }
      seen[(size_t)dst[k]] = 1;
    }
  }
  const int W = L.window;
  const RgStateField *f_rt = L.find("reset_time"), *f_fsum = L.find("fsum"), *f_fcorr = L.find("fcorr"), *f_lat = L.find("latched"),
                     *f_swq = L.find("swing_q"), *f_flags = L.find("flags"), *f_ld = L.find("last_desired"), *f_rl = L.find("ring_len"),
                     *f_rh = L.find("ring_head"), *f_sv = L.find("swing_valid"), *f_wk = L.find("warm_key"), *f_wc = L.find("ws_cnt"),
                     *f_hard = L.find("hard"), *f_ncs = L.find("ncs"), *f_it = L.find("iters"), *f_ring = L.find("ring"),
                     *f_wz = L.find("warm_z"), *f_wy = L.find("warm_y"), *f_ids = L.find("ws_ids");
  for (k = 0; k < n; k++) {
    const unsigned char *r = (const unsigned char *)rows + (size_t)k * L.row_words * 4;
    auto u32 = [&](int word) { uint32_t v; memcpy(&v, r + 4 * (size_t)word, 4); return v; };
    auto i32 = [&](const RgStateField *f, int i) { int32_t v; memcpy(&v, r + 4 * (size_t)f->word + 4 * (size_t)i, 4); return v; };
    auto f32 = [&](const RgStateField *f, int i) { float v; memcpy(&v, r + 4 * (size_t)f->word + 4 * (size_t)i, 4); return (double)v; };
    auto f64 = [&](const RgStateField *f, int i) { double v; memcpy(&v, r + 4 * (size_t)f->word + 8 * (size_t)i, 8); return v; };
    auto finite = [](double v) { return (bool)std::isfinite(v); };
    if (u32(0) != RG_STATE_MAGIC) return bad("header", "magic %.0f is not a state row", (double)u32(0));
    if (u32(1) != RG_STATE_VERSION) return bad("header", "version %.0f is not this library's", (double)u32(1));
    if (((uint64_t)u32(3) << 32 | u32(2)) != L.hash) return bad("header", "layout hash %.0f differs from this layout's (window, horizon or field list)", (double)u32(2));
    const int rlen = i32(f_rl, 0), rhead = i32(f_rh, 0), wc = i32(f_wc, 0), wk = i32(f_wk, 0), sv = i32(f_sv, 0);
    if (rlen < 0 || rlen > W) return bad("ring_len", "= %.0f outside [0, window]", rlen);
    if (rhead < 0 || rhead >= W) return bad("ring_head", "= %.0f outside [0, window)", rhead);
    if (wc < 0 || wc > RG_STATE_WS_MAX) return bad("ws_cnt", "= %.0f outside [0, RG_WS_MAX]", wc);
    for (int i = 0; i < RG_STATE_WS_MAX; i++) {
      const int id = r[4 * (size_t)f_ids->word + i];
      if (id >= L.ws_id_limit) return bad("ws_ids", "entry = %.0f not below the constraint count of the horizon", id);
    }
    if (wk < -1 || wk > 15) return bad("warm_key", "= %.0f outside [-1, 15]", wk);
    if (i32(f_hard, 0) < 0 || i32(f_hard, 0) > 16) return bad("hard", "= %.0f outside [0, 16]", i32(f_hard, 0));
    if (i32(f_ncs, 0) < 0 || i32(f_ncs, 0) > 4) return bad("ncs", "= %.0f outside [0, 4]", i32(f_ncs, 0));
    if (i32(f_it, 0) < 0 || i32(f_it, 0) > (1 << 24)) return bad("iters", "= %.0f outside [0, 2^24]", i32(f_it, 0));
    if (i32(f_flags, 0) & ~3) return bad("flags", "= %.0f uses undefined bits", i32(f_flags, 0));
    if (i32(f_ld, 0) & ~0xF) return bad("last_desired", "= %.0f uses undefined bits", i32(f_ld, 0));
    if (sv & ~0xFFF) return bad("swing_valid", "= %.0f uses undefined bits", sv);
    if (!finite(f64(f_rt, 0))) return bad("reset_time", "= %g is not finite", f64(f_rt, 0));
    for (int i = 0; i < 3; i++) {
      if (!finite(f64(f_fsum, i))) return bad("fsum", "= %g is not finite", f64(f_fsum, i));
      if (!finite(f64(f_fcorr, i))) return bad("fcorr", "= %g is not finite", f64(f_fcorr, i));
    }
    for (int i = 0; i < 12; i++) {
      if (!finite(f64(f_lat, i))) return bad("latched", "= %g is not finite", f64(f_lat, i));
      // a joint whose swing_valid bit is clear has no stored angle yet: the step never reads it
      if (((sv >> i) & 1) && !finite(f64(f_swq, i))) return bad("swing_q", "= %g is not finite where swing_valid is set", f64(f_swq, i));
    }
    // the velocity window: the ring_len samples before ring_head are summed; the other slots are written before they are read
    for (int j = 0; j < rlen; j++) {
      const int slot = ((rhead - 1 - j) % W + W) % W;
      for (int a = 0; a < 3; a++)
        if (!finite(f32(f_ring, a * W + slot))) return bad("ring", "sample = %g is not finite", f32(f_ring, a * W + slot));
    }
    // the stored iterate is read only while warm_key names a contact set
    if (wk >= 0)
      for (int i = 0; i < RG_WARM_N; i++) {
        if (!finite(f32(f_wz, i))) return bad("warm_z", "= %g is not finite", f32(f_wz, i));
        if (!finite(f32(f_wy, i))) return bad("warm_y", "= %g is not finite", f32(f_wy, i));
      }
  }
  return true;
}

// ------------------------------------------------------------------------------------
// device side
// ------------------------------------------------------------------------------------
struct StateMap {
  uint32_t *base[RG_STATE_MAX_FIELDS];   // the handle's array of each field (null: the handle has none -- saved as zeros, not loaded)
  int word[RG_STATE_MAX_FIELDS], words[RG_STATE_MAX_FIELDS], esz[RG_STATE_MAX_FIELDS], rm[RG_STATE_MAX_FIELDS];
  int nf, words_c, row_words, rt_word;
  uint32_t hdr[RG_STATE_HDR_WORDS];
};

// (robot slot k, word w) of thread t: component-major words first (lane = robot), then robot-major ones (lane = word)
__device__ __forceinline__ bool state_thread(const StateMap &S, const int n, int &k, int &w) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long nc = (long long)n * S.words_c;
  if (t < nc) {
    w = (int)(t / n);
    k = (int)(t - (long long)w * n);
    return true;
  }
  const int wr = S.row_words - S.words_c;
  const long long u = t - nc;
  if (u >= (long long)n * wr) return false;
  k = (int)(u / wr);
  w = S.words_c + (int)(u - (long long)k * wr);
  return true;
}

// the field that holds word w (w >= header), selected with constant indices only (a per-lane index into the kernel
// arguments would copy them to scratch); the same field for most lanes of a wave
struct StateSel { uint32_t *base; int word, words, esz, rm; };
__device__ __forceinline__ StateSel state_field(const StateMap &S, const int w) {
  StateSel s{S.base[0], S.word[0], S.words[0], S.esz[0], S.rm[0]};
#pragma unroll
  for (int i = 1; i < RG_STATE_MAX_FIELDS; i++)
    if (i < S.nf && S.word[i] <= w) s = StateSel{S.base[i], S.word[i], S.words[i], S.esz[i], S.rm[i]};
  return s;
}

__device__ __forceinline__ uint32_t *state_addr(const StateSel &f, const int w, const int b, const int B) {
  const int o = w - f.word;
  if (f.rm) return f.base + (size_t)b * f.words + o;
  const int c = o / f.esz, h = o - c * f.esz;
  return f.base + ((size_t)c * B + b) * f.esz + h;
}

__global__ void __launch_bounds__(256) rg_state_gather_kernel(const StateMap S, const int *__restrict__ idx, const int n, const int B,
                                                              uint32_t *__restrict__ rows) {
  int k, w;
  if (!state_thread(S, n, k, w)) return;
  const int b = idx ? idx[k] : k;
  if (b < 0 || b >= B) return;
  uint32_t v = 0;
  if (w < RG_STATE_HDR_WORDS) {
#pragma unroll
    for (int i = 0; i < RG_STATE_HDR_WORDS; i++)
      if (w == i) v = i == 4 ? (uint32_t)b : S.hdr[i];
  } else {
    const StateSel f = state_field(S, w);
    if (f.base) v = *state_addr(f, w, b, B);
  }
  rows[(size_t)k * S.row_words + w] = v;
}

__global__ void __launch_bounds__(256) rg_state_scatter_kernel(const StateMap S, const int *__restrict__ idx, const int n, const int B,
                                                               const uint32_t *__restrict__ rows, const double *__restrict__ shift) {
  int k, w;
  if (!state_thread(S, n, k, w) || w < RG_STATE_HDR_WORDS) return;
  const int b = idx ? idx[k] : k;
  if (b < 0 || b >= B) return;
  const StateSel f = state_field(S, w);
  if (!f.base) return;
  const uint32_t *src = rows + (size_t)k * S.row_words;
  if (shift && w == S.rt_word) {   // resume on a new clock: the lane of the first word writes the shifted value
    const double t0 = __hiloint2double((int)src[w + 1], (int)src[w]);
    *(double *)state_addr(f, w, b, B) = t0 + shift[k];
    return;
  }
  if (shift && w == S.rt_word + 1) return;
  *state_addr(f, w, b, B) = src[w];
}

static StateMap state_map(const RgStateLayout &L, const DevState &st) {
  StateMap S{};
  S.nf = L.nfields; S.words_c = L.words_c; S.row_words = L.row_words;
  for (int i = 0; i < L.nfields; i++) {
    const RgStateField &f = L.f[i];
    const char *nm = f.name;
    void *p = nullptr;
    if (!strcmp(nm, "reset_time")) p = st.reset_time;
    else if (!strcmp(nm, "fsum")) p = st.fsum;
    else if (!strcmp(nm, "fcorr")) p = st.fcorr;
    else if (!strcmp(nm, "latched")) p = st.latched;
    else if (!strcmp(nm, "swing_q")) p = st.swing_q;
    else if (!strcmp(nm, "flags")) p = st.flags;
    else if (!strcmp(nm, "last_desired")) p = st.last_desired;
    else if (!strcmp(nm, "ring_len")) p = st.ring_len;
    else if (!strcmp(nm, "ring_head")) p = st.ring_head;
    else if (!strcmp(nm, "swing_valid")) p = st.swing_valid;
    else if (!strcmp(nm, "cmd")) p = st.cmd;
    else if (!strcmp(nm, "warm_key")) p = st.warm_key;
    else if (!strcmp(nm, "ws_cnt")) p = st.ws_cnt;
    else if (!strcmp(nm, "hard")) p = st.hard;
    else if (!strcmp(nm, "ncs")) p = st.ncs;
    else if (!strcmp(nm, "iters")) p = st.iters;
    else if (!strcmp(nm, "ring")) p = st.ring;
    else if (!strcmp(nm, "warm_z")) p = st.warm_z;
    else if (!strcmp(nm, "warm_y")) p = st.warm_y;
    else if (!strcmp(nm, "ws_ids")) p = st.ws_ids;
    S.base[i] = (uint32_t *)p;
    S.word[i] = f.word; S.words[i] = f.words; S.rm[i] = f.robot_major;
    S.esz[i] = f.kind == 0 ? 2 : 1;
    if (!strcmp(nm, "reset_time")) S.rt_word = f.word;
  }
  S.hdr[0] = RG_STATE_MAGIC; S.hdr[1] = RG_STATE_VERSION;
  S.hdr[2] = (uint32_t)(L.hash & 0xffffffffu); S.hdr[3] = (uint32_t)(L.hash >> 32);
  return S;
}

static dim3 state_grid(const RgStateLayout &L, int n) {
  return dim3((unsigned)(((long long)n * L.row_words + 255) / 256));
}

hipError_t rg_state_gather(const RgStateLayout &L, const DevState &st, int B, const int *idx, int n, long long steps, uint32_t *rows,
                           hipStream_t s) {
  if (n <= 0) return hipSuccess;
  StateMap S = state_map(L, st);
  S.hdr[5] = (uint32_t)(steps & 0x7fffffff);
  hipLaunchKernelGGL(rg_state_gather_kernel, state_grid(L, n), dim3(256), 0, s, S, idx, n, B, rows);
  return hipGetLastError();
}

hipError_t rg_state_scatter(const RgStateLayout &L, const DevState &st, int B, const int *idx, int n, const uint32_t *rows,
                            const double *shift, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  const StateMap S = state_map(L, st);
  hipLaunchKernelGGL(rg_state_scatter_kernel, state_grid(L, n), dim3(256), 0, s, S, idx, n, B, rows, shift);
  return hipGetLastError();
}

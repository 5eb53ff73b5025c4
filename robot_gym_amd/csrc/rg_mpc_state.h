// rg_mpc_state.h -- state rows (rg_mpc_save_state / rg_mpc_load_state / rg_mpc_copy_state): the row layout, the host
// validator and the launchers of the gather / scatter kernels in rg_mpc_state.hip.  Host declarations only: rg_mpc.hip
// includes this file, and none of its kernels changes.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <string>

struct DevState;
struct DevCfg;

#define RG_STATE_MAGIC 0x54534752u   // "RGST"
#define RG_STATE_VERSION 1
#define RG_STATE_HDR_WORDS 8         // magic, version, layout hash (2), saved-from robot, handle step count, 2 reserved
#define RG_STATE_WS_MAX 64           // = RG_WS_MAX (rg_qp_exact_kernel.inc; rg_mpc.hip asserts it)
#define RG_STATE_MAX_FIELDS 24

// One field of the row.  kind: 0 float64, 1 float32, 2 int32, 3 uint8.  robot_major: the device array is [B][count] (warm
// start, working set); otherwise it is component-major [count][B].  word: first 32-bit word of the field in the row.
struct RgStateField {
  const char *name;
  int kind, count, robot_major, word, words;
};

struct RgStateLayout {
  int window = 0, horizon = 0;
  int nfields = 0;
  RgStateField f[RG_STATE_MAX_FIELDS];
  int words_c = 0;        // header + component-major fields (lane = robot in the kernels)
  int row_words = 0;      // ... + robot-major fields (lane = word)
  uint64_t hash = 0;
  std::string desc;
  int ws_id_limit = 0;    // constraint ids of a stored working set are below this (6 per force block, exact bodies)
  const RgStateField *find(const char *name) const;
};

// window >= 1, horizon 10 or 20; false (and err) otherwise
bool rg_state_layout_build(int window, int horizon, RgStateLayout *L, std::string &err);

// Validates n host rows against L: header, ranges, bit masks and finite values.  dst (may be null): the robots the rows go
// to, checked against [0, batch) and for repeats.  false: err names the first bad entry, its robot and the field.
bool rg_state_validate(const RgStateLayout &L, const void *rows, int n, const int32_t *dst, int batch, std::string &err);

// Device side (rg_mpc_state.hip).  idx: device array of n robot indices (null: robots 0..n-1).
// gather: n rows of the handle's state -> rows (device, n * row_words words); header words from hash / steps.
// scatter: n rows (device) -> the handle's state; shift (device, may be null): added to reset_time of row k.
hipError_t rg_state_gather(const RgStateLayout &L, const DevState &st, int B, const int *idx, int n, long long steps,
                           uint32_t *rows, hipStream_t s);
hipError_t rg_state_scatter(const RgStateLayout &L, const DevState &st, int B, const int *idx, int n, const uint32_t *rows,
                            const double *shift, hipStream_t s);

// rg_reset_kernel's work (rg_reset_body.inc) for every robot b with mask[b] != 0; mask: device int32 [B].  Enqueued on s,
// no staging, no wait.  The kernel and this launcher are in rg_episode.hip: the kernel sets of rg_mpc.hip and rg_mpc_state.hip
// are pinned by tests.
hipError_t rg_state_reset_masked(const DevCfg *cfg_dev, const DevState &st, int B, const int *mask, double t0, hipStream_t s);

/*
 * rg_srb_terrain.h -- the terrain entries of the C-ABI of the batched single-rigid-body simulator.  Part of rg_srb.h, which
 * includes this file at its end and states the ground, the three rules it changes and the conventions at its top; include
 * rg_srb.h, not this file.
 */
#ifndef RG_SRB_TERRAIN_H
#define RG_SRB_TERRAIN_H

#ifndef RG_SRB_H
#error "include rg_srb.h"
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define RG_SRB_TERRAIN_FLAT 0
#define RG_SRB_TERRAIN_RANDOM 1
#define RG_SRB_TERRAIN_GRID 2
#define RG_SRB_TERRAIN_MAX_DIM 4096

/* The ground (see the top of this file).  The caller owns key and heights and keeps them alive while the terrain is set. */
typedef struct {
  int32_t abi_version;      /* RG_SRB_ABI_VERSION */
  int32_t kind;             /* RG_SRB_TERRAIN_* */
  double cell;              /* vertex spacing, m: > 0 (random, grid) */
  double amplitude;         /* random: heights in [0, amplitude); >= 0 */
  uint64_t seed;            /* random */
  const int64_t *key;       /* random: [B] device, or NULL = key 0 for every robot; must be NULL otherwise */
  const double *heights;    /* grid: [rows][cols] device; must be NULL otherwise */
  int32_t rows, cols;       /* grid: 2 .. RG_SRB_TERRAIN_MAX_DIM; 0 otherwise */
  double x0, y0;            /* grid: where heights[0][0] sits; 0 otherwise */
  int64_t reserved[4];      /* must be 0 */
} rg_srb_terrain;

int32_t rg_srb_terrain_size(void);

/* 0 if t is a valid terrain, else RG_SRB_ERR_INVALID with the text (it names the field) in msg[0..n).  Needs no device and
 * no handle: abi_version, a known kind, reserved fields 0; random and grid: cell finite and > 0; random: amplitude finite
 * and >= 0, no heights, rows = cols = 0, x0 = y0 = 0; grid: heights given, rows and cols in range, x0 and y0 finite, no key,
 * amplitude and seed 0; flat: every other field 0 / NULL.  msg may be NULL. */
int rg_srb_terrain_check(const rg_srb_terrain *t, char *msg, int32_t n);

/* Sets the ground of a handle; validated by rg_srb_terrain_check before anything changes.  NULL or kind 0 returns the handle
 * to the plane.  rg_srb_step and rg_srb_reset dispatch on it.  Does not touch any state: call rg_srb_settle, or reset. */
int rg_srb_set_terrain(rg_srb_handle *h, const rg_srb_terrain *t);

/* out[k] = h(xy[k], xy[n + k]; robot[k]) of the handle's ground (0.0 on the plane).  xy [2][n], out [n] float64 and robot
 * [n] int32 (each in [0, B); one outside is taken as the nearest robot) are DEVICE arrays; robot NULL: entry k is robot k and n <= B. */
int rg_srb_ground_height(rg_srb_handle *h, const double *xy, const int32_t *robot, int32_t n, double *out, void *stream);

/* Settle (see the top of this file) of the robots b with mask[b] != 0 (mask: int32 [B] DEVICE array, or NULL: all) whose
 * status is 0; every other robot is left untouched.  On the plane every height is 0.0.  Never synchronises. */
int rg_srb_settle(rg_srb_handle *h, double *state, const int32_t *mask, const rg_srb_obs_ptrs *obs, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* RG_SRB_TERRAIN_H */

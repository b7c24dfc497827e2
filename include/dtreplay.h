/* dtreplay.h — C-ABI of the GPU prioritized replay.
 *
 * Replaces, for the batched DDPG path, the index side of
 *   utils/buffers.py:140-259   PrioritizedReplayBuffer (add / sample / update_priorities)
 *   utils/segment_tree.py:94-146 SumSegmentTree + MinSegmentTree
 * The payload (observations, actions, ...) lives in caller-owned device tensors
 * indexed by the slots these calls return (aido1_amd/replay.py).
 *
 * Layout in HBM: two float64 trees of 2*capacity nodes each (node 1 = root,
 * leaf i at capacity + i, as segment_tree.py:34), an int32[capacity] scratch
 * used to resolve duplicate indices in one update, and the float64 running
 * max priority.  All state stays on the device: add / sample / update are
 * stream-ordered and never synchronise.
 *
 * Conventions as dtsim.h: every call returns 0 or a negative DT_E_* code,
 * device pointers belong to the handle's GPU, work goes on `stream`
 * (a hipStream_t, NULL = default stream).
 */
#ifndef AIDO1_AMD_DTREPLAY_H
#define AIDO1_AMD_DTREPLAY_H

#include <stdint.h>

#include "dtsim.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dt_per dt_per;

/* PrioritizedReplayBuffer(size, alpha) — buffers.py:141-167: capacity = next
 * power of two >= size, sum tree 0, min tree +inf, max_priority 1. */
int dt_per_create(int64_t size, double alpha, int32_t device, dt_per** out);
void dt_per_destroy(dt_per* h);
const char* dt_per_last_error(const dt_per* h);
int64_t dt_per_capacity(const dt_per* h);
int64_t dt_per_len(const dt_per* h);      /* len(buffer._storage) */
int64_t dt_per_next_idx(const dt_per* h); /* buffer._next_idx */

/* n consecutive add() calls — buffers.py:169-174 + ReplayBuffer.add :29-36:
 * slot k = (next_idx + k) % size gets leaf max_priority**alpha in both trees.
 * slots_dev (int64[n], may be NULL) receives each add's slot; when n > size
 * later adds overwrite earlier ones, so the payload of add k belongs in
 * slots[k] only if k >= n - size. */
int dt_per_add(dt_per* h, int64_t n, int64_t* slots_dev, void* stream);

/* sample(batch, beta) — buffers.py:176-235 with random.random() replaced by
 * u_dev[batch] (float64 in [0,1)): mass = u * sum(0, len - 1) (leaves
 * 0..len-2, the reference's reduce() end quirk), idx = find_prefixsum_idx(mass)
 * (segment_tree.py:106-132), weight = (p_idx * len)^-beta / (p_min * len)^-beta.
 * Needs len >= 2 (the reference recurses forever at len 1). */
int dt_per_sample(dt_per* h, int32_t batch, const double* u_dev, double beta, int64_t* idx_dev,
                  double* weights_dev, void* stream);

/* update_priorities(idx, priorities) — buffers.py:237-259: leaf = p**alpha
 * (the last occurrence of a duplicated index wins, as the sequential loop),
 * max_priority = max(max_priority, p).  Entries the reference would reject
 * (p <= 0 or NaN, idx outside [0, len)) are skipped, flagged and counted
 * for dt_per_check. */
int dt_per_update(dt_per* h, int32_t n, const int64_t* idx_dev, const double* priorities_dev,
                  void* stream);

/* dt_per_update with priorities |td[i]| + eps (td device float32 [n], the
 * trainer's TD errors; the float32 absolute value widened to float64, then
 * + eps: what update_priorities(idx, abs(td) + eps) stores). */
int dt_per_update_td(dt_per* h, int32_t n, const int64_t* idx, const float* td, double eps,
                     void* stream);

/* Copy out the trees (float64[2*capacity] each; NULL to skip) and the max
 * priority (float64[1]) — tests and checkpointing. */
int dt_per_read(dt_per* h, double* sum_dev, double* min_dev, double* max_priority_dev,
                void* stream);

/* Synchronises; DT_E_ARG if an update since the last check held an entry the
 * reference's asserts reject (message in dt_per_last_error: the kinds and how
 * many entries were skipped). */
int dt_per_check(dt_per* h);

/* dt_frame_add: one decision of the frame store behind
 * ReplayBuffer.add_batch_ring (aido1_amd/replay.py, frame_envs).  Replaces the
 * two stacked observation copies buffers.py:29-36 stores per transition
 * (obs_t, obs_tp1; the Transformer stack of 3 frames each): a decision adds
 * ONE frame per env, and a transition keeps frame-row indices instead.
 *   src        device, env e's newest frame at src + e * src_env_stride
 *              4-byte words (the rollout ring's newest slot); frames are copied
 *              as opaque words: f32 grey, or 4 u8 palette-index pixels a word
 *              (dt_render_io.index); frame_elems words a frame, a multiple of
 *              4, src and dst 16-B aligned
 *   dst        device [n, frame_elems] words: frame rows base_row .. base_row + n - 1
 *   stack      device int32 [n, k]: each env's current stack as frame rows
 *              (oldest first), advanced in place
 *   done       device uint8 [n] or NULL: respawned envs, whose whole stack
 *              becomes the new row (the renderer refilled every slot)
 *   obs_ptr    device int32 [n, k] out: the stack before (the transition's obs)
 *   next_ptr   device int32 [n, k] out: the stack after (its next_obs) */
int dt_frame_add(int32_t n, int64_t frame_elems, const void* src, int64_t src_env_stride,
                 void* dst, int32_t k, int32_t* stack, const uint8_t* done, int32_t base_row,
                 int32_t* obs_ptr, int32_t* next_ptr, void* stream);

/* dt_frame_gather: a sampled batch of the frame store straight into the
 * update's inputs (ReplayBuffer._encode_sample, buffers.py:38-52, then
 * DDPGTrainer's float32 channels_last inputs, trainers.py:156-163), one
 * launch instead of the index_selects, the layout change, the casts and the
 * copies into the captured graph's static inputs.  For b < batch, i = idx[b]:
 *   obs[b][y][x][c] = frames[obs_ptr[i][c]][y * w + x]   (c < k; NHWC: the
 *   nxt[b][y][x][c] = frames[next_ptr[i][c]][...]         channels_last memory
 *                                                          of [batch, k, h, w])
 *   act[b][j] = action[i][j] (j < 2), rew[b] = (float)reward[i],
 *   notdone[b] = done[i] ? 0 : 1
 *   idx device i64 [batch] in [0, size) (unchecked: dt_per_sample's output);
 *   frames [rows, hw]: frame_kind 0 f32 grey, 1 u8 palette-index frames
 *   (dt_render_io.index), decoded through dt_palette_gray's table (so the
 *   output equals kind 0's on the grey frames bit for bit); obs_ptr /
 *   next_ptr i32 [size, k]; action f32 [size, 2]; reward f64 [size]; done u8
 *   [size] (torch bool); k <= 4 */
int dt_frame_gather(int32_t batch, const int64_t* idx, const void* frames, int32_t frame_kind,
                    int64_t hw, int32_t k, const int32_t* obs_ptr, const int32_t* next_ptr,
                    const float* action, const double* reward, const uint8_t* done, float* obs,
                    float* nxt, float* act, float* rew, float* notdone, void* stream);

/* dt_frame_gather plus the batch's importance weights in the same launch:
 * w[b] = (float)weights[b], weights device f64 [batch] (dt_per_sample's
 * weights_dev: indexed by batch position, not by slot), w device f32 [batch]
 * (the trainer's static 'w' input).  Both NULL: dt_frame_gather; exactly one
 * NULL: DT_E_ARG. */
int dt_frame_gather_w(int32_t batch, const int64_t* idx, const void* frames, int32_t frame_kind,
                      int64_t hw, int32_t k, const int32_t* obs_ptr, const int32_t* next_ptr,
                      const float* action, const double* reward, const uint8_t* done, float* obs,
                      float* nxt, float* act, float* rew, float* notdone, const double* weights,
                      float* w, void* stream);

/* ---- device replay of the batched train-ddpg-cnn.py rollout (aido1_amd/cnn_replay.py) ----
 * New entry points only: no existing signature or layout changes, so
 * DT_ABI_VERSION stays 14.
 *
 * duckietown_rl/utils.py:18-57 (ReplayBuffer) in slot form.  Transition s (the
 * 0-based count of every add) takes slot s while s < max_size; later it evicts
 * slot (w * max_size) >> 32 (64-bit), w = word 0 of philox4x32_10((lo32(s),
 * hi32(s), 0, 'EVIC' = 0x45564943), (lo32(seed), hi32(seed))).  Draw d (the
 * count of every draw) reads slot (w * len) >> 32, w from the block tagged
 * 'SMPL' = 0x534D504C with d in s's place.  A transition is six palette-index
 * byte frames (state 0-2, next_state 3-5, each newest first) and 16 B of
 * scalars.  All five calls are stateless, validate on the host (DT_E_ARG
 * before any launch) and never synchronise. */

/* n adds with serials added .. added + n - 1.  owner: device u64 [max_size],
 * zero at creation, never cleared: each lane does atomicMax(owner[slot],
 * s + 1), then rows[i] (device i64 [n]) = slot where owner[slot] == s + 1,
 * else -1: of two adds of this batch to one slot the later keeps it, as
 * sequential adds would leave it.  Afterwards owner[slot] - 1 is the serial
 * the slot holds.  1 <= max_size < 2^31. */
int dt_replay_claim(int32_t n, int64_t added, int64_t max_size, uint64_t seed, uint64_t* owner,
                    int64_t* rows, void* stream);

/* The byte twin of dt_stack_take (dtactor.h): for every env e < n with
 * mask[e] != 0 (mask NULL: every env) and rows[e] >= 0,
 *   frames[rows[e]][3 * half + j] = ring[e][order[j]]   (j < 3, 19,200 B verbatim)
 * ring: device u8 [n, slots, 120, 160] (an index ring), frames: device u8
 * [max_size, 6, 120, 160], both 16-B aligned; order[3] host, each in
 * [0, slots); half 0 (state) or 1 (next_state). */
int dt_stack_store(const uint8_t* ring, int32_t n, int32_t slots, const int32_t* order,
                   const uint8_t* mask, const int64_t* rows, int32_t half, uint8_t* frames,
                   void* stream);

/* The scalars of the envs with rows[e] >= 0: act_store[rows[e]] = action[e]
 * (f32 x 2), rew_store = (float)repeat_reward[e] (f64 -> f32, as
 * ddpg.ReplayBuffer stores it), done_store = done_float[e]. */
int dt_replay_commit(int32_t n, const int64_t* rows, const float* action,
                     const double* repeat_reward, const float* done_float, float* act_store,
                     float* rew_store, float* done_store, void* stream);

/* Draws drawn .. drawn + batch - 1 over len = min(added, max_size) filled
 * slots into idx (device i64 [batch]).  1 <= len < 2^31. */
int dt_replay_draw(int32_t batch, int64_t drawn, int64_t len, uint64_t seed, int64_t* idx,
                   void* stream);

/* The sampled batch in the layout ddpg.DDPG.train reads: obs / nxt float32
 * [batch, 3, 120, 160] = dt_palette_gray's table over frames[idx[b]][0..2] /
 * [3..5] (bit for bit dt_stack_take's decode), as planes (nhwc == 0) or in
 * channels-last memory (nhwc != 0: obs[b][y][x][c]); act [batch, 2], rew
 * [batch, 1], done [batch, 1] copied.  idx device i64 [batch], unchecked
 * (dt_replay_draw's or dt_replay_claim's output), may repeat a slot.  frames,
 * obs and nxt 16-B aligned. */
int dt_cnn_replay_gather(int32_t batch, const int64_t* idx, const uint8_t* frames,
                         const float* act_store, const float* rew_store, const float* done_store,
                         int32_t nhwc, float* obs, float* nxt, float* act, float* rew,
                         float* done, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* AIDO1_AMD_DTREPLAY_H */

// Shared pieces of the actor's convolution kernels: dtconv.hip (fp16 MFMA,
// the fast mode) and dtconvx.hip (the same chain at float32 accuracy on fp16
// MFMA, "x3").  Types, the LeakyReLU form, the two-weight-set split of a
// persistent grid, the per-sample centring of reference-mode outputs, the
// row-stream geometry (RowStream) with its step index and step loop, the
// per-sample statistics (Welford, Chan's merge, the exact two-pass form),
// conv1's frame-ring loader and weight gather, and the launchers' argument
// checks.
#ifndef AIDO1_AMD_DTCONV_COMMON_H
#define AIDO1_AMD_DTCONV_COMMON_H

#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "../../include/dtactor.h"

namespace dtconv {

using half8 = __attribute__((ext_vector_type(8))) _Float16;
using f32x16 = __attribute__((ext_vector_type(16))) float;
using u32x4 = __attribute__((ext_vector_type(4))) uint32_t;

constexpr int CO = 32;   // output channels of every conv of the actor

// LeakyReLU for 0 <= s <= 1 as two instructions (a multiply and a max)
__device__ __forceinline__ float lrelu2(float v, float s) { return fmaxf(v, v * s); }

// Reference mode keeps each sample's activations CENTRED: the stored value is
// v - c with c the sample's pixel-0 output of the channel, and the statistics
// are those of the stored values (M2 does not change, the mean moves by c), so
// the next layer's norm (x - mean) * invstd is unchanged.  A channel that is
// nearly flat over a frame is divided by a tiny standard deviation; stored
// uncentred its rounding (~2^-11 |v| in fp16) is amplified by that 1 / std,
// centred the rounding is of |v - c| ~ the channel's own spread.  The sample's
// first step publishes c (wave 0, pixel 0 = lanes 0 and 32) and a barrier
// makes it visible; later steps read it (rewritten only after the step barrier
// that ends the sample).  `first` is workgroup-uniform.  Register r of a
// 32x32 MFMA tile holds channel (r & 3) + 8 (r >> 2) + 4 h (h = lane half).
__device__ __forceinline__ void centre_px32(float (&v)[16], float* s_c, bool publish, bool first,
                                            int h) {
  if (publish)
#pragma unroll
    for (int r = 0; r < 16; ++r) s_c[(r & 3) + 8 * (r >> 2) + 4 * h] = v[r];
  if (first) __syncthreads();
#pragma unroll
  for (int r = 0; r < 16; ++r) v[r] -= s_c[(r & 3) + 8 * (r >> 2) + 4 * h];
}

// ---- two weight sets in one launch -----------------------------------------------
// Samples [0, n0) use the launch's weights, [n0, n) a second set (the exploiting
// explorers' actor): the persistent workgroups split in proportion, g0 for the
// first set, the rest for the second, and each loads only its own set.  One set:
// n0 = n, g0 = gridDim.x.
struct WeightSplit {
  int n0, g0;
  const void* wfrag;
  const float *bias, *in_gamma, *in_beta, *out_gamma, *out_beta;
};
struct SplitPart {
  bool set2;
  int bid, gdim, sbeg, send, my;   // this WG's index / count in its part, its samples
};
__device__ __forceinline__ SplitPart split_part(const WeightSplit& ws, int n) {
  SplitPart p;
  p.set2 = (int)blockIdx.x >= ws.g0;
  p.bid = p.set2 ? (int)blockIdx.x - ws.g0 : (int)blockIdx.x;
  p.gdim = p.set2 ? (int)gridDim.x - ws.g0 : ws.g0;
  p.sbeg = p.set2 ? ws.n0 : 0;
  p.send = p.set2 ? n : ws.n0;
  const int nloc = p.send - p.sbeg;
  p.my = nloc > p.bid ? (nloc - p.bid + p.gdim - 1) / p.gdim : 0;
  return p;
}
// device: a second-set workgroup's parameters re-pointed at its set
template <typename W>
__device__ __forceinline__ void use_set2(const WeightSplit& ws, const W* __restrict__& wfrag,
                                         const float* __restrict__& bias,
                                         const float* __restrict__& in_gamma,
                                         const float* __restrict__& in_beta,
                                         const float* __restrict__& out_gamma,
                                         const float* __restrict__& out_beta) {
  wfrag = static_cast<const W*>(ws.wfrag);
  bias = ws.bias;
  in_gamma = ws.in_gamma;
  in_beta = ws.in_beta;
  out_gamma = ws.out_gamma;
  out_beta = ws.out_beta;
}
// host: the grid of a launch over n samples (n0 of them with the first set) on
// `grid` resident workgroups; fills ws.n0 / ws.g0
inline int split_grid(WeightSplit& ws, int n, int n0, int grid) {
  if (n0 <= 0 || n0 >= n) {   // one set
    ws.n0 = n;
    ws.g0 = n < grid ? n : grid;
    return ws.g0;
  }
  int g0 = (int)(((long long)grid * n0 + n / 2) / n);
  g0 = g0 < 1 ? 1 : (g0 > grid - 1 ? grid - 1 : g0);
  const int g1raw = grid - g0;
  ws.n0 = n0;
  ws.g0 = n0 < g0 ? n0 : g0;
  const int g1 = (n - n0) < g1raw ? (n - n0) : g1raw;
  return ws.g0 + g1;
}
// host: the second set of a launch from the C ABI's dt_conv_set (NULL: one set,
// all zero); n0 / g0 are split_grid's
inline WeightSplit weight_split(const dt_conv_set* set2) {
  WeightSplit ws{};
  if (set2) {
    ws.wfrag = set2->wfrag;
    ws.bias = set2->bias;
    ws.in_gamma = set2->in_gamma;
    ws.in_beta = set2->in_beta;
    ws.out_gamma = set2->out_gamma;
    ws.out_beta = set2->out_beta;
  }
  return ws;
}

// host: a second set's own checks (n0 in range, weights and bias, and the
// norm parameters the launch reads)
inline bool set2_ok(const dt_conv_set* set2, int n, bool need_in, bool need_out) {
  if (!set2) return true;
  if (set2->n0 < 0 || set2->n0 > n || !set2->wfrag || !set2->bias) return false;
  if (need_in && (!set2->in_gamma || !set2->in_beta)) return false;
  return !need_out || (set2->out_gamma && set2->out_beta);
}
// host: the arguments every conv1 launch takes
inline bool conv1_args_ok(const void* ring, int n, int slots, const int32_t* order,
                          const void* wfrag, const float* bias, const dt_conv_set* set2,
                          const void* y) {
  if (!ring || !wfrag || !bias || !y || !order || n < 0 || slots < 3) return false;
  for (int i = 0; i < 3; ++i)
    if (order[i] < 0 || order[i] >= slots) return false;
  return set2_ok(set2, n, false, false);
}

// ---- row-stream geometry ------------------------------------------------------------
// A persistent workgroup of NW waves streams whole samples (IH x IW in, a KH-row
// kernel at stride ST, OH x OW out) through a ring of input rows in LDS; a step
// is NW tiles of 32 consecutive output pixels, one per wave.
template <int IH_, int IW_, int OH_, int OW_, int ST, int KH, int NW_>
struct RowStream {
  static constexpr int IH = IH_, OW = OW_, NW = NW_;
  static constexpr int kPix = OH_ * OW_;
  static constexpr int kTiles = (kPix + 31) / 32;
  static constexpr int kSteps = (kTiles + NW - 1) / NW;
  static constexpr int kStepPix = 32 * NW;
  // input rows step j reads: lo(j) .. hi(j)
  __host__ __device__ static constexpr int lo(int j) { return ST * ((kStepPix * j) / OW); }
  __host__ __device__ static constexpr int hi(int j) {
    const int end = kStepPix * (j + 1) < kPix ? kStepPix * (j + 1) : kPix;
    const int r = ST * ((end - 1) / OW) + KH - 1;
    return r < IH - 1 ? r : IH - 1;
  }
  // the rows the step after j adds: first_new(j) .. last_new(j) (its earlier
  // rows are already in the ring; the last step of a sample adds the next
  // sample's first rows)
  __host__ __device__ static constexpr int first_new(int j) {
    return (j + 1 == kSteps) ? 0 : (hi(j) + 1 > lo(j + 1) ? hi(j) + 1 : lo(j + 1));
  }
  __host__ __device__ static constexpr int last_new(int j) {
    return (j + 1 == kSteps) ? hi(0) : hi(j + 1);
  }
  // ring rows: step j's rows and its successor's held at once
  static constexpr int ring() {
    int m = 0;
    for (int j = 0; j < kSteps; ++j) {
      const int span = (j + 1 < kSteps) ? hi(j + 1) - lo(j) + 1 : (IH - lo(j)) + hi(0) + 1;
      m = span > m ? span : m;
    }
    return m;
  }
  // most rows one step's prefetch brings in
  static constexpr int max_new() {
    int m = 0;
    for (int j = 0; j < kSteps; ++j) {
      const int r = last_new(j) - first_new(j) + 1;
      m = r > m ? r : m;
    }
    return m;
  }
};

// Where step (k, j) of a stream S stands: the two steps after it
struct StepIdx {
  bool last_j, last_j1;   // step g / step g+1 is the last of its sample
  int k1, j1, k2;         // step g+1 is (k1, j1); step g+2 belongs to sample k2
};
template <typename S>
__device__ __forceinline__ StepIdx step_idx(int k, int j) {
  StepIdx s;
  s.last_j = j + 1 == S::kSteps;
  s.k1 = s.last_j ? k + 1 : k;
  s.j1 = s.last_j ? 0 : j + 1;
  s.last_j1 = s.j1 + 1 == S::kSteps;
  s.k2 = s.last_j1 ? s.k1 + 1 : s.k1;
  return s;
}
// This wave's tile of step j: lane `col` has output pixel p = (oy, ox) of pc,
// p clamped to the sample.  Apart from step_idx so that a kernel can place
// it after the step's prefetch loads: the compiler keeps it where it is
// written.
struct TileIdx {
  int p, pc, oy, ox;
  bool valid;
};
template <typename S>
__device__ __forceinline__ TileIdx tile_idx(int j, int wave, int col) {
  TileIdx t;
  const int tile = S::NW * j + wave;
  t.p = 32 * tile + col;
  t.valid = t.p < S::kPix;
  t.pc = t.valid ? t.p : 0;
  t.oy = t.pc / S::OW;
  t.ox = t.pc - t.oy * S::OW;
  return t;
}
// The steps g = 0 .. total - 1 of a workgroup, two an iteration so that the
// prefetch register sets pa / pb swap roles at compile time: step(g, k, j,
// nxt, cur) with (k, j) the step's sample and its step in it.
template <int kSteps, typename Buf, typename F>
__device__ __forceinline__ void run_steps(int total, Buf& pa, Buf& pb, F&& step) {
  int k = 0, j = 0;
  for (int g = 0; g < total; g += 2) {
    step(g, k, j, pa, pb);
    if (++j == kSteps) { j = 0; ++k; }
    if (g + 1 < total) {
      step(g + 1, k, j, pb, pa);
      if (++j == kSteps) { j = 0; ++k; }
    }
  }
}

// ---- per-sample statistics -----------------------------------------------------------
// One more value a channel into a lane's Welford state.  kRcp: 1 / count as
// v_rcp_f32 (1 ulp: an O(1e-7) relative weight error).
template <bool kRcp>
__device__ __forceinline__ void welford_add(const float (&v)[16], float& w_cnt,
                                            float (&w_mean)[16], float (&w_m2)[16]) {
  w_cnt += 1.0f;
  const float inv = kRcp ? __builtin_amdgcn_rcpf(w_cnt) : 1.0f / w_cnt;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const float d = v[r] - w_mean[r];
    w_mean[r] += d * inv;
    w_m2[r] += d * (v[r] - w_mean[r]);
  }
}
// Chan's merge of the waves' (count, mean, M2) of channel tid in red
struct Moments {
  float cnt, mean, m2;
};
template <int NW>
__device__ __forceinline__ Moments chan_merge(const float (*red)[CO][3], int tid) {
  float cnt = 0.0f, mean = 0.0f, m2 = 0.0f;
  for (int w = 0; w < NW; ++w) {
    const float nb = red[w][tid][0];
    if (nb <= 0.0f) continue;
    const float tot = cnt + nb, d = red[w][tid][1] - mean;
    mean += d * (nb / tot);
    m2 += red[w][tid][2] + d * d * (cnt * nb / tot);
    cnt = tot;
  }
  return {cnt, mean, m2};
}
// a wave's per-channel (count, mean, M2) of a 32x32 tile into red (lanes col 0)
__device__ __forceinline__ void red_put(float (*red)[CO][3], int wave, int h, float cnt,
                                        const float (&mean)[16], const float (&m2)[16]) {
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int c = (r & 3) + 8 * (r >> 2) + 4 * h;
    red[wave][c][0] = cnt;
    red[wave][c][1] = mean[r];
    red[wave][c][2] = m2[r];
  }
}
// Per-lane Welford statistics of a 32x32 tile's 16 channels merged over the
// sample: the lanes of each half (shuffles), then the waves (red, one
// barrier), written as (mean, M2, c) per channel to the sample's 3 CO floats
// at out by threads < CO.
template <int NW>
__device__ __forceinline__ void stats_flush(float& w_cnt, float (&w_mean)[16], float (&w_m2)[16],
                                            float (*red)[CO][3], const float* s_c, float* out,
                                            int tid, int wave, int col, int h) {
#pragma unroll
  for (int o = 1; o < 32; o <<= 1) {
    const float nb = __shfl_xor(w_cnt, o, 32);
    const float tot = w_cnt + nb;
    const float fa = tot > 0.0f ? nb / tot : 0.0f, fb = tot > 0.0f ? w_cnt * nb / tot : 0.0f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float mb = __shfl_xor(w_mean[r], o, 32), m2b = __shfl_xor(w_m2[r], o, 32);
      const float d = mb - w_mean[r];
      w_mean[r] += d * fa;
      w_m2[r] += m2b + d * d * fb;
    }
    w_cnt = tot;
  }
  if (col == 0) red_put(red, wave, h, w_cnt, w_mean, w_m2);
  __syncthreads();
  if (tid < CO) {
    const Moments m = chan_merge<NW>(red, tid);
    float* pp = out + tid * 3;
    pp[0] = m.mean;
    pp[1] = m.m2;
    pp[2] = s_c[tid];
  }
  w_cnt = 0.0f;
#pragma unroll
  for (int r = 0; r < 16; ++r) w_mean[r] = w_m2[r] = 0.0f;
}
// Exact two-pass statistics of a sample held in one step: per wave, two
// passes over its own 32 pixels (shuffles only: exact mean, then M2 about
// it); the waves' (n, mean, M2) merged with Chan's formula by threads < CO,
// which hand them to fin(Moments); two barriers a sample.  Level by level
// over the 16 channels: each level's 16 shuffles are in flight together
// (channel by channel, every shuffle waited for the one before it: 160
// dependent LDS round trips, 16k cycles a sample); each channel's sums keep
// their order, so the bits are unchanged.
template <int NW, typename F>
__device__ __forceinline__ void twopass_stats(const float (&v)[16], bool valid,
                                              float (*red)[CO][3], int tid, int wave, int col,
                                              int h, F fin) {
  float nw = valid ? 1.0f : 0.0f;
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) nw += __shfl_xor(nw, o, 32);
  const float inw = nw > 0.0f ? 1.0f / nw : 0.0f;
  float sum[16], m2[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) sum[r] = valid ? v[r] : 0.0f;
#pragma unroll
  for (int o = 16; o > 0; o >>= 1)
#pragma unroll
    for (int r = 0; r < 16; ++r) sum[r] += __shfl_xor(sum[r], o, 32);
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const float d = valid ? v[r] - sum[r] * inw : 0.0f;
    m2[r] = d * d;
  }
#pragma unroll
  for (int o = 16; o > 0; o >>= 1)
#pragma unroll
    for (int r = 0; r < 16; ++r) m2[r] += __shfl_xor(m2[r], o, 32);
  if (col == 0) {
#pragma unroll
    for (int r = 0; r < 16; ++r) sum[r] *= inw;   // the wave's means
    red_put(red, wave, h, nw, sum, m2);
  }
  __syncthreads();
  if (tid < CO) fin(chan_merge<NW>(red, tid));
  __syncthreads();
}

// the two half-waves' 4-channel groups of a 32x32 tile's registers paired
// (v_permlane32_swap), so that a lane holds 8 consecutive channels; several
// register sets are exchanged pair by pair, interleaved
template <typename... U>
__device__ __forceinline__ void swap_halves(U&... u) {
  auto one = [](uint32_t& a, uint32_t& b) __attribute__((always_inline)) {
    const auto r = __builtin_amdgcn_permlane32_swap(a, b, false, false);
    a = r[0];
    b = r[1];
  };
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int e = 0; e < 2; ++e) (one(u[2 * m][e], u[2 * m + 1][e]), ...);
}

// ---- conv1's row stream ------------------------------------------------------------
// 120x160 input, 8x8 stride 2 -> 57x77, kSW waves; the ring holds kSRing rows
// of 3-channel fp16 pixels (K 192: 12 MFMAs a tile, in groups of 3 a kernel
// row pair).
namespace c1 {
constexpr int IH = 120, IW = 160, OH = 57, OW = 77;
constexpr int kSW = 4;
using Stream = RowStream<IH, IW, OH, OW, 2, 8, kSW>;
constexpr int kSThreads = 64 * kSW;
constexpr int kSPix = Stream::kPix;                          // 4389
constexpr int kSTiles = Stream::kTiles;
constexpr int kSSteps = Stream::kSteps;
constexpr int kSRing = 32;                              // rows (a power of two)
constexpr int kSQuads = IW / 4;                         // 4-pixel load items per row
constexpr int kSPre = (Stream::max_new() * kSQuads + kSThreads - 1) / kSThreads;
constexpr int kSPxB = 6;                                // bytes a ring pixel: fp16 x 3
constexpr int kSRowB = IW * kSPxB;                      // 960 B
constexpr int kSMfma = 12, kSGrp = 3;                   // MFMAs a tile, a B-fragment group
static_assert(kSTiles == 138 && kSSteps == 35 && Stream::ring() == 18 && kSPre == 2);
static_assert(Stream::ring() <= kSRing, "conv1 stream ring");

// kIdx: the frame ring holds palette-index frames (u8): a load item is one
// 32-bit word of 4 pixels a frame instead of a float4
template <bool kIdx> using Elem = typename std::conditional<kIdx, uint8_t, float>::type;
template <bool kIdx> using Item = typename std::conditional<kIdx, uint32_t, float4>::type;
// a thread's load items are fixed (row r, quad q - r kSQuads of the step's
// range); only the range start and length change per step
struct Items {
  int r[kSPre], off[kSPre], lds[kSPre];   // row, element offset in the frame, byte in the ring row
};
__device__ __forceinline__ Items items(int tid) {
  Items it;
#pragma unroll
  for (int i = 0; i < kSPre; ++i) {
    const int q = tid + i * kSThreads;
    it.r[i] = q / kSQuads;
    it.off[i] = it.r[i] * IW + 4 * (q - it.r[i] * kSQuads);
    it.lds[i] = 4 * kSPxB * (q - it.r[i] * kSQuads);
  }
  return it;
}
struct NoCheck {
  __device__ __forceinline__ void operator()(const void*) const {}
};
// Rows r0..r1 of sample s (clamped below send) into registers, one item per
// stacked frame s0..s2; every load issued on every path (items past the range
// re-load the range's first quad), so the compiler's vmcnt waits stay exact.
// A step may add no rows (r0 = r1 + 1, up to IH at the end of a sample): its
// loads then read the sample's row 0, never past the plane.  check(p) sees
// every address loaded from (diagnostic builds).
template <bool kIdx, typename Check = NoCheck>
__device__ __forceinline__ void issue(Item<kIdx> (&pre)[kSPre][3], const Items& it,
                                      const Elem<kIdx>* ringT, int slots, int s0, int s1, int s2,
                                      int s, int send, int r0, int r1, Check check = {}) {
  constexpr size_t plane = (size_t)IH * IW;
  const int rows = r1 - r0 + 1;
  const int ns = s < send ? s : send - 1;
  const Elem<kIdx>* base = ringT + (size_t)ns * slots * plane + (size_t)(rows > 0 ? r0 : 0) * IW;
  const Elem<kIdx>* p0 = base + (size_t)s0 * plane;
  const Elem<kIdx>* p1 = base + (size_t)s1 * plane;
  const Elem<kIdx>* p2 = base + (size_t)s2 * plane;
#pragma unroll
  for (int i = 0; i < kSPre; ++i) {
    const int off = it.r[i] < rows ? it.off[i] : 0;
    check(p0 + off);
    pre[i][0] = *reinterpret_cast<const Item<kIdx>*>(p0 + off);
    check(p1 + off);
    pre[i][1] = *reinterpret_cast<const Item<kIdx>*>(p1 + off);
    check(p2 + off);
    pre[i][2] = *reinterpret_cast<const Item<kIdx>*>(p2 + off);
  }
}
// A fragments: MFMA s covers kernel rows ky = 2(s/3) + h (h = the lane half)
// and 8 of the 24 (kx, c) values of a row, t = 8(s%3) + j -> kx = t/3,
// c = t%3: a lane's 8 k are 16 contiguous bytes of a ring row.  Gathered once
// from the dt_conv1 fragment layout (include/dtactor.h) at wh.
__device__ __forceinline__ void gather_a(half8 (&wa)[kSMfma], const _Float16* wh) {
  const int lane = threadIdx.x & 63, co = lane & 31, hh = lane >> 5;
#pragma unroll
  for (int s = 0; s < kSMfma; ++s)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int ky = 2 * (s / 3) + hh, t = 8 * (s % 3) + e, kx = t / 3, c = t % 3;
      const int s1 = 2 * ky + kx / 4, l1 = co + 32 * ((kx & 3) >> 1), j1 = 4 * (kx & 1) + c;
      wa[s][e] = wh[(s1 * 64 + l1) * 8 + j1];
    }
}
}  // namespace c1

// resident workgroups a CU of `kern` at `threads` (the persistent grids)
template <typename K>
inline int resident_grid(K kern, int threads, int cap) {
  int dev = 0, cus = 256, per = 1;
  if (hipGetDevice(&dev) == hipSuccess)
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, kern, threads, 0) != hipSuccess || per < 1)
    per = 1;
  if (cap > 0 && cap < per) per = cap;
  return per * cus;
}

}  // namespace dtconv

#endif  // AIDO1_AMD_DTCONV_COMMON_H

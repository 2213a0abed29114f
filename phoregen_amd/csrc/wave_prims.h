// Wave-level primitives shared by the attention, adjoint and streaming-GEMM kernels: cross-lane moves and row reductions, the folded
// LayerNorm of a K-path tile, the bounded sin/cos, the LDS-DMA load, and the constants those kernels must agree on.
#pragma once
#include "common.h"

namespace pg {

typedef int i4v __attribute__((ext_vector_type(4)));

// softmax floor: the logit of a masked row and the start of a running max (a logit <= 0.5 * NEG_BIG gets weight 0)
constexpr float NEG_BIG = -1.0e30f;

// angular features of the triplet update (models/common.py:67-87 with duplicated sin/cos(theta) columns merged)
__device__ __constant__ const float kAngFreq[12] = {0.f, 1.f, 2.f, 3.f, 0.5f, (float)(1.0 / 3.0), 1.f, 2.f, 3.f, 0.5f,
                                                    (float)(1.0 / 3.0), 0.f};

template <int CTRL>
__device__ __forceinline__ float dpp_mov(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
// sum / max over the 16 lanes of a DPP row (lanes with equal lane>>4); every lane ends up with the result
__device__ __forceinline__ float row16_total(float v) {
  v += dpp_mov<0xB1>(v);    // quad_perm [1,0,3,2]
  v += dpp_mov<0x4E>(v);    // quad_perm [2,3,0,1]
  v += dpp_mov<0x141>(v);   // row_half_mirror
  v += dpp_mov<0x140>(v);   // row_mirror
  return v;
}
__device__ __forceinline__ float row16_max(float v) {
  v = fmaxf(v, dpp_mov<0xB1>(v));
  v = fmaxf(v, dpp_mov<0x4E>(v));
  v = fmaxf(v, dpp_mov<0x141>(v));
  v = fmaxf(v, dpp_mov<0x140>(v));
  return v;
}
// max / min / sum over all 64 lanes, every lane ends up with the result: a fixed butterfly, so the result depends on the lanes'
// values alone (call with the whole wave active)
__device__ __forceinline__ float wave_max(float v) {
  v = row16_max(v);
  v = fmaxf(v, __shfl_xor(v, 16));
  return fmaxf(v, __shfl_xor(v, 32));
}
__device__ __forceinline__ float wave_min(float v) { return -wave_max(-v); }
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ int wave_imax(int v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = max(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ int wave_imin(int v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = min(v, __shfl_xor(v, o));
  return v;
}
// v of lane src_lane (any lane of the wave, ds_bpermute)
__device__ __forceinline__ float from_lane(float v, int src_lane) {
  return __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(src_lane << 2, __builtin_bit_cast(int, v)));
}

// LDS written by some lanes of a wave and read by others: order the accesses without a workgroup barrier
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Folded LayerNorm + ReLU (packing._kv_mlp: hidden is centred and sign-normalised, |gamma| lives in the next Linear):
// z = ReLU(hidden + b' * sigma); returns 1/sigma, which the caller applies to the row's logits / attention weights.
// K-path tile: hid[tau][r] = hidden[c = 16 tau + 4g + r][row = m]
__device__ __forceinline__ float ln_relu_kpath(f4 (&hid)[8], const float* bp, int g) {
  float q = 0.f;
#pragma unroll
  for (int tq = 0; tq < 8; ++tq)
#pragma unroll
    for (int r = 0; r < 4; ++r) q = fmaf(hid[tq][r], hid[tq][r], q);
  q += __shfl_xor(q, 16);
  q += __shfl_xor(q, 32);
  const float var = q * (1.f / 128.f) + 1e-5f;
  const float rs = __builtin_amdgcn_rsqf(var);
  const float sigma = var * rs;
#pragma unroll
  for (int tq = 0; tq < 8; ++tq) {
    const f4 bt = *reinterpret_cast<const f4*>(bp + 16 * tq + 4 * g);
#pragma unroll
    for (int r = 0; r < 4; ++r) hid[tq][r] = fmaxf(fmaf(bt[r], sigma, hid[tq][r]), 0.f);
  }
  return rs;
}

// Bounded sin / cos for 0 <= arg <= ~10 (the angular code arguments are bounded by 3 pi): k = rint(arg * 2/pi), r = arg - k pi/2 by a
// two-constant Cody-Waite reduction, then ps = sin(r) (degree 9) and pc = cos(r) (degree 8) on [-pi/4, pi/4]; returns the quadrant
// k (+ 1 with `next`: cos(x) is the sine one quadrant on, exactly).  The triplet forward and its adjoints must evaluate exactly this
// arithmetic: the one-pass adjoints reuse the forward's softmax weights.
__device__ __forceinline__ int sincos_reduce(float arg, bool next, float& ps, float& pc) {
  const float kf = rintf(arg * 0.63661977236758134308f);
  float r = fmaf(-kf, 1.57079637050628662109375f, arg);
  r = fmaf(-kf, -4.37113900018624283e-8f, r);
  const int q = (int)kf + (next ? 1 : 0);
  const float s = r * r;
  ps = fmaf(s, 2.7557314297e-6f, -1.9841270114e-4f);
  ps = fmaf(ps, s, 8.3333337680e-3f);
  ps = fmaf(ps, s, -1.6666667163e-1f);
  ps = fmaf(ps * s, r, r);
  pc = fmaf(s, 2.4801587642e-5f, -1.3888889225e-3f);
  pc = fmaf(pc, s, 4.1666667908e-2f);
  pc = fmaf(pc, s, -0.5f);
  pc = fmaf(pc, s, 1.0f);
  return q;
}
// sin(arg) or cos(arg): quadrant select
__device__ __forceinline__ float sincos_bounded(float arg, bool want_cos) {
  float ps, pc;
  const int q = sincos_reduce(arg, want_cos, ps, pc) & 3;
  const float v = (q & 1) ? pc : ps;
  return (q & 2) ? -v : v;
}
// sin(arg) and cos(arg) from one reduction: quadrant rotation
__device__ __forceinline__ void sincos_bounded_pair(float arg, float& sn, float& cs) {
  float ps, pc;
  const int q = sincos_reduce(arg, false, ps, pc);
  const float a = (q & 1) ? pc : ps, b = (q & 1) ? ps : pc;       // sin(arg) = +-a, cos(arg) = +-b
  sn = (q & 2) ? -a : a;
  cs = ((q + 1) & 2) ? -b : b;
}

// raw buffer descriptor over `bytes` at `base` (wave-uniform; stride 0: byte offsets)
__device__ __forceinline__ i4v raw_buffer_desc(const void* base, unsigned bytes) {
  const unsigned long long a = reinterpret_cast<unsigned long long>(base);
  i4v d;
  d[0] = __builtin_amdgcn_readfirstlane((int)(a & 0xffffffffu));
  d[1] = __builtin_amdgcn_readfirstlane((int)((a >> 32) & 0xffffu));
  d[2] = __builtin_amdgcn_readfirstlane((int)bytes);
  d[3] = 0x00020000;
  return d;
}
// One 1 KB piece HBM -> LDS without registers (LDS-DMA): lane l's 16 bytes from base + voff + soff land at LDS byte address lds_dst + 16 l.
// The compiler pads nothing inside an asm string and does not keep M0 across one, so the statement carries its own wait states: `s_nop 4`
// because desc / soff may come straight from v_readfirstlane (a VALU-written SGPR needs five states before a buffer instruction reads
// it), M0 (the LDS destination base) written in the statement that uses it, `s_nop 0` between that write and the load.  The load is not
// in the compiler's s_waitcnt bookkeeping either: the caller retires it with a counted vmcnt wait before the LDS is read.
__device__ __forceinline__ void lds_dma_1k(unsigned lds_dst, unsigned voff, i4v desc, unsigned soff) {
  asm volatile("s_nop 4\n\ts_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds"
               :: "s"(lds_dst), "v"(voff), "s"(desc), "s"(soff) : "memory");
}

}  // namespace pg

// ppoconv.hip — the PPO cnn agent's ConvBlock (ppo/agent.py:45-103: 1 -> 128, then 128 -> 128,
// all 3x3, stride 1, padding 1 on 7x7 boards, each followed by Dropout and ReLU) on the device:
// the 128 -> 128 layers on split-f16 MFMA products (the leaf net's "x3" arithmetic, fp32-class),
// forward, input gradient (the same kernel on flipped / transposed weights) and weight gradient;
// the 1 -> 128 layer in plain fp32; the dropout's keep bits and the activation gradient.
// Activations are NHWC f32 [B][7][7][128]: the dense buffer of a channels_last [B,128,7,7] tensor.
//
// k_conv7_x3: persistent, one workgroup of 4 waves per CU walking tiles of kC7T = 8 boards
// (tile = blockIdx.x, += gridDim.x; the last tile may be partial). The tile's boards share one
// zero-haloed LDS grid of 65 rows x 9 slots of 16 B per plane: row 0 zero, then per board 7 rows
// and one zero row (shared between neighbours); column 0 and column 8 zero. 392 pixels = 24.5
// MFMA groups of 16, padded to 25 (a multiple of kLnSlots); the pixel -> slot map is the greedy
// of LnPixMap (16 slots distinct mod 16 per group: the row stride 9 is odd, so the classes are
// balanced). Wave w owns output blocks 2w and 2w + 1 (32 channels: 2 x 25 accumulators = 200
// AGPRs), each B fragment feeds both. K = 36 chunks (9 taps x 4 quarters of 32 input channels);
// the input channels are staged in two halves of 64 (16 planes of 9472 B = 148 KB of LDS), each
// through 100 VGPRs; the first pass over the tile also takes the board maxima over both halves,
// the second half is read again (an L2 hit) when it is staged. Every board has its own power-of-two scale
// (largest magnitude into [2^14, 2^15)), applied when it is staged and removed in the epilogue
// by the board of the accumulator's column.
// Epilogue: y = acc * inv[o] * 2^-ex(board) + bias[o], then (optional) * keep bit * keep_scale,
// then (optional) ReLU; NHWC store.
#include "../../include/blokus_engine.h"
#include "ctx.h"

#include "leafnet_common.h"

namespace bk {
namespace {

constexpr int kC7T = 8;                    // boards per tile
constexpr int kC7RS = 9;                   // grid row stride in slots
constexpr int kC7Rows = 1 + 8 * kC7T;      // 65 grid rows
constexpr int kC7Px = 49 * kC7T;           // 392 pixels per tile
constexpr int kC7NG = 25;                  // MFMA column groups (400 columns, 8 spare)
constexpr int kC7PL = (kC7Rows * kC7RS * 16 + 255) / 256 * 256;  // plane bytes (9472)
constexpr int kC7Lds = 16 * kC7PL + 128;   // 16 planes + board maxima [8] + board exponents [8]
constexpr int kC7Chunks = 36;
constexpr int kC7WBytes = kC7Chunks * 8 * 2 * kBlock * 2;  // [chunk 36][block 8][part 2][lane 64][8] f16
// The f16 MFMA's accumulation rounds toward -inf by a small fraction of an ulp of the running sum
// (measured on 800 K outputs against fp64: mean error -0.065 of the rms error with signed operands,
// -0.11 with positive ones, proportional to the accumulator's magnitude; the fp32 convolution's
// mean error is zero). The bias is harmless per element but adds up in sums over many outputs
// (bias gradients). From chunk kC7Flip of the second channel half on (2/3 of K) the kernel
// accumulates the negated sum (accumulators negated once, then negated weights), whose bias has
// the other sign, so the two parts cancel to first order; the epilogue's scale carries the sign.
constexpr int kC7Flip = 6;
static_assert(kC7NG % kLnSlots == 0 && kC7NG * 16 >= kC7Px, "k_conv7_x3: groups");
static_assert(kC7Lds <= 160 * 1024, "k_conv7_x3: LDS");

__host__ __device__ constexpr int c7_slot(int p) {  // tile pixel -> grid slot
  return (1 + (p / 49) * 8 + (p % 49) / 7) * kC7RS + (p % 49) % 7 + 1;
}
__device__ __forceinline__ int c7_pixel(int slot) {  // grid slot -> tile pixel
  const int r1 = slot / kC7RS - 1, col = slot % kC7RS - 1;
  return (r1 >> 3) * 49 + (r1 & 7) * 7 + col;
}

// LnPixMap's greedy on the tile's grid: each group takes one pixel per slot class mod 16 where
// the classes allow, leftovers fill the gaps; -1 = spare column.
struct C7PixMap {
  int slot[kC7NG * 16];
  constexpr C7PixMap() : slot() {
    bool used[kC7Px] = {};
    for (int i = 0; i < kC7NG * 16; ++i) slot[i] = -1;
    for (int g = 0; g < kC7NG; ++g)
      for (int r = 0; r < 16; ++r)
        for (int p = 0; p < kC7Px; ++p) {
          const int sl = c7_slot(p);
          if (!used[p] && sl % 16 == r) {
            used[p] = true;
            slot[g * 16 + r] = sl;
            break;
          }
        }
    int p = 0;
    for (int i = 0; i < kC7NG * 16; ++i) {
      if (slot[i] >= 0) continue;
      while (p < kC7Px && used[p]) ++p;
      if (p == kC7Px) break;
      used[p] = true;
      slot[i] = c7_slot(p);
    }
  }
};
__device__ constexpr C7PixMap kC7PixMap{};

// ln_chunk for two output blocks that share the B fragments: per group 6 MFMAs, the two
// accumulators interleaved (acc0 += a0h bh, acc1 += a1h bh, acc0 += a0l bh, acc1 += a1l bh,
// acc0 += a0h bl, acc1 += a1h bl); the ring and its read-ahead are ln_chunk's.
template <int NG, int HALF>
__device__ __forceinline__ void c7_chunk(f32x4 (&acc0)[NG], f32x4 (&acc1)[NG], h16x8 a0h, h16x8 a0l, h16x8 a1h,
                                         h16x8 a1l, const unsigned char* grid, const int (&pb)[NG], int coff,
                                         int coff_next, h16x8 (&rb)[kLnSlots][2]) {
  static_assert(NG % kLnSlots == 0, "c7_chunk: the ring slot of a group must not depend on the chunk");
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    const int gp = g + kLnPf;
    if (gp < NG)
      ln_load<HALF>(rb[gp % kLnSlots], grid, pb[gp], coff);
    else
      ln_load<HALF>(rb[gp % kLnSlots], grid, pb[gp - NG], coff_next);
    const h16x8 bh = rb[g % kLnSlots][0], bl = rb[g % kLnSlots][1];
    asm volatile(
        "v_mfma_f32_16x16x32_f16 %0, %2, %4, %0\n\t"
        "v_mfma_f32_16x16x32_f16 %1, %5, %4, %1\n\t"
        "v_mfma_f32_16x16x32_f16 %0, %3, %4, %0\n\t"
        "v_mfma_f32_16x16x32_f16 %1, %6, %4, %1\n\t"
        "v_mfma_f32_16x16x32_f16 %0, %2, %7, %0\n\t"
        "v_mfma_f32_16x16x32_f16 %1, %5, %7, %1"
        : "+a"(acc0[g]), "+a"(acc1[g])
        : "v"(a0h), "v"(a0l), "v"(bh), "v"(a1h), "v"(a1l), "v"(bl));
  }
}

// the fused epilogue's tail: v * (keep bit ? keep_scale : 0), then ReLU; bits = the 4 keep bits
// of v's channels (all ones without a mask)
__device__ __forceinline__ f32x4 c7_act(f32x4 v, unsigned bits, bool masked, float keep_scale, int relu) {
  if (masked) {
    v.x = (bits & 1u) ? v.x * keep_scale : 0.0f;
    v.y = (bits & 2u) ? v.y * keep_scale : 0.0f;
    v.z = (bits & 4u) ? v.z * keep_scale : 0.0f;
    v.w = (bits & 8u) ? v.w * keep_scale : 0.0f;
  }
  if (relu) {
    v.x = max_bits(v.x, 0);
    v.y = max_bits(v.y, 0);
    v.z = max_bits(v.z, 0);
    v.w = max_bits(v.w, 0);
  }
  return v;
}

__global__ __launch_bounds__(kLnThreads, 1) void k_conv7_x3(const float* __restrict__ x, const h16x8* __restrict__ w,
                                                            const float* __restrict__ inv,
                                                            const float* __restrict__ bias,
                                                            const unsigned* __restrict__ keep, float keep_scale,
                                                            int relu, float* __restrict__ y, int B) {
  constexpr int RS = kC7RS, NG = kC7NG, PL = kC7PL;
  constexpr int HQ = kC7Px * 16;                             // float4 quads per channel half of a tile
  constexpr int HIT = (HQ + kLnThreads - 1) / kLnThreads;    // 25 (the last one half full)
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  unsigned char* act = lds;  // 16 planes [hi | lo][65 x 9 slots][16 B] of the staged channel half
  unsigned* bmax = reinterpret_cast<unsigned*>(lds + 16 * PL);  // [8] board maxima (float bits)
  int* bex = reinterpret_cast<int*>(lds + 16 * PL + 32);        // [8] board exponents
  const int tid = threadIdx.x, l = tid & 63, n = l & 15, ks = l >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int oc = 32 * wave + 4 * ks;  // block 2 wave: channels oc..oc+3, block 2 wave + 1: oc + 16..

  // zero the grid once: every tile writes the interiors only (absent boards as zeros)
  for (int i = tid; i < 16 * PL / 16; i += kLnThreads) reinterpret_cast<u32x4*>(lds)[i] = u32x4{0u, 0u, 0u, 0u};
  if (tid < 8) bmax[tid] = 0u;
  __syncthreads();

  constexpr int kBias = (RS + 1) * 16;
  int ab[NG];
  unsigned valid = 0;
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    const int sl = kC7PixMap.slot[16 * g + n];
    ab[g] = (sl >= 0 ? sl : RS + 1) * 16 + ks * 4 * PL - kBias;
    valid |= (sl >= 0 ? 1u : 0u) << g;
  }
  const __amdgpu_buffer_rsrc_t wrs = ln_rsrc(w, (unsigned)kC7WBytes);
  auto wload = [&](int chunk, int j, int part) {
    return __builtin_bit_cast(
        h16x8, __builtin_amdgcn_raw_buffer_load_b128(wrs, l * 16, ((chunk * 8 + 2 * wave + j) * 2 + part) * 1024, 0));
  };
  // (negated: the accumulators end up holding the negated sums, kC7Flip)
  const f32x4 sv0 = -*reinterpret_cast<const f32x4*>(inv + oc), sv1 = -*reinterpret_cast<const f32x4*>(inv + oc + 16);
  const f32x4 zero4{0.f, 0.f, 0.f, 0.f};
  const f32x4 bv0 = bias ? *reinterpret_cast<const f32x4*>(bias + oc) : zero4;
  const f32x4 bv1 = bias ? *reinterpret_cast<const f32x4*>(bias + oc + 16) : zero4;
  auto coff_of = [&](int c) {  // chunk c of a half: tap c / 2, quarter c % 2 of the half
    const int t = c >> 1;
    return 2 * (c & 1) * PL + ((t / 3 - 1) * RS + (t % 3 - 1)) * 16 + kBias;
  };

  const int ntiles = (B + kC7T - 1) / kC7T;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const size_t px0 = (size_t)tile * kC7Px;  // the tile's first pixel
    const int npx = min(kC7Px, (B - tile * kC7T) * 49);
    // channel half 0 of the tile into registers (item i = quad tid + 256 i) and, in the same pass,
    // the per-board maxima over both halves (half 1 is read again, from the L2, when it is staged);
    // a wave's 64 quads are 4 consecutive pixels, in at most two boards
    // (the thread and wave ids pass through empty asm statements per tile: the per-item addresses
    // are then computed where they are used instead of being hoisted out of the tile loop, which
    // would hold a hundred registers and more across the MFMA phase)
    f32x4 xv[HIT];
    int t0 = tid, wv = wave;
    asm volatile("" : "+v"(t0), "+s"(wv));
    auto load = [&](int h) {
#pragma unroll
      for (int i = 0; i < HIT; ++i) {
        const int q = t0 + i * kLnThreads, p = q >> 4, qq = q & 15;
        const bool ok = q < HQ && p < npx;
        const f32x4* src = reinterpret_cast<const f32x4*>(x + (px0 + (size_t)p) * 128) + h * 16 + qq;
        xv[i] = ok ? *src : zero4;
      }
    };
    load(0);
#pragma unroll
    for (int i = 0; i < HIT; ++i) {
      const int q = t0 + i * kLnThreads, p = q >> 4, qq = q & 15;
      const bool ok = q < HQ && p < npx;
      const f32x4 x1 = ok ? *(reinterpret_cast<const f32x4*>(x + (px0 + (size_t)p) * 128) + 16 + qq) : zero4;
      const int p_lo = (wv * 64 + i * kLnThreads) >> 4;
      const int bd = min(p / 49, kC7T - 1), bd_lo = min(p_lo / 49, kC7T - 1), bd_hi = min((p_lo + 3) / 49, kC7T - 1);
      float m = max3_abs(max3_abs(0.0f, xv[i].x, xv[i].y), xv[i].z, xv[i].w);
      m = max3_abs(max3_abs(m, x1.x, x1.y), x1.z, x1.w);
      const float m_lo = wave_max_f(bd == bd_lo ? m : 0.0f);
      if (l == 0) atomicMax(&bmax[bd_lo], __builtin_bit_cast(unsigned, m_lo));
      if (bd_hi != bd_lo) {  // wave-uniform
        const float m_hi = wave_max_f(bd == bd_hi ? m : 0.0f);
        if (l == 0) atomicMax(&bmax[bd_hi], __builtin_bit_cast(unsigned, m_hi));
      }
    }
    __syncthreads();  // the maxima are complete; every wave is done with the previous tile
    if (tid < kC7T) {
      bex[tid] = scale_exp(__builtin_bit_cast(float, bmax[tid]));
      bmax[tid] = 0u;
    }
    __syncthreads();

    f32x4 acc0[NG], acc1[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) acc0[g] = acc1[g] = zero4;

#pragma unroll 1
    for (int h = 0; h < 2; ++h) {
      if (h == 1) {
        asm volatile("" : "+v"(t0));
        load(1);
        __syncthreads();  // the first half's grid reads are done
      }
      // scale by the board's power of two, split, into the planes: quad qq of pixel p = channels
      // 64 h + 4 qq.., octet o = qq / 2 (hi plane 4 (o % 4) + 2 (o / 4), lo the next)
#pragma unroll
      for (int i = 0; i < HIT; ++i) {
        const int q = t0 + i * kLnThreads, p = q >> 4, qq = q & 15, o = qq >> 1;
        if (q < HQ) {
          const f32x4 v = xv[i];
          const int ex = bex[p / 49];
          unsigned h0, h1, l0, l1;
          split2(ldexpf(v.x, ex), ldexpf(v.y, ex), h0, l0);
          split2(ldexpf(v.z, ex), ldexpf(v.w, ex), h1, l1);
          unsigned char* d = act + ((o & 3) * 4 + (o >> 2) * 2) * PL + c7_slot(p) * 16 + (qq & 1) * 8;
          *reinterpret_cast<u32x2*>(d) = u32x2{h0, h1};
          *reinterpret_cast<u32x2*>(d + PL) = u32x2{l0, l1};
        }
      }
      __syncthreads();

      // the half's 18 chunks (tap c / 2, quarter 2 h + c % 2), weights one chunk ahead
      h16x8 wq[2][4];
      auto wchunk = [&](h16x8 (&d)[4], int c) {
        const int chunk = (c >> 1) * 4 + 2 * h + (c & 1);
        d[0] = wload(chunk, 0, 0);
        d[1] = wload(chunk, 0, 1);
        d[2] = wload(chunk, 1, 0);
        d[3] = wload(chunk, 1, 1);
      };
      wchunk(wq[0], 0);
      h16x8 rb[kLnSlots][2];
      ln_prime<NG, PL>(rb, act, ab, coff_of(0));
#pragma unroll
      for (int c = 0; c < 18; ++c) {
        if (c + 1 < 18) wchunk(wq[(c + 1) & 1], c + 1);
        if (c == kC7Flip && h == 1) {  // from here on the accumulators hold the negated sums (see kC7Flip)
          ln_mfma_drain(acc0);
          ln_mfma_drain(acc1);
#pragma unroll
          for (int g = 0; g < NG; ++g) {  // one group at a time through VGPRs (the volatile asms keep the order)
            f32x4 t0 = acc0[g], t1 = acc1[g];
            asm volatile("" : "+v"(t0), "+v"(t1));
            acc0[g] = -t0;
            acc1[g] = -t1;
            asm volatile("" : "+a"(acc0[g]), "+a"(acc1[g]));
          }
          asm volatile("s_nop 7\n\ts_nop 7" ::: "memory");  // AGPR writes -> the MFMAs' srcC
        }
        const unsigned sgn = (h == 1 && c >= kC7Flip) ? 0x80008000u : 0u;
        h16x8 wc[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const u32x4 u = __builtin_bit_cast(u32x4, wq[c & 1][j]);
          wc[j] = __builtin_bit_cast(h16x8, u32x4{u.x ^ sgn, u.y ^ sgn, u.z ^ sgn, u.w ^ sgn});
        }
        c7_chunk<NG, PL>(acc0, acc1, wc[0], wc[1], wc[2], wc[3], act, ab, coff_of(c), coff_of(c + 1 < 18 ? c + 1 : c),
                         rb);
      }
    }
    ln_mfma_drain(acc0);
    ln_mfma_drain(acc1);

    // y = acc * inv * 2^-ex(board) + bias (* keep * keep_scale, ReLU), NHWC
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      if (!((valid >> g) & 1u)) continue;
      int sb = ab[g];
      asm volatile("" : "+v"(sb));  // as above: the pixel of column g is computed here, per tile
      const int p = c7_pixel((sb - ks * 4 * PL + kBias) / 16);
      if (p >= npx) continue;
      const int ex = bex[p / 49];
      const size_t gp = px0 + (size_t)p;
      unsigned kb0 = 0xFu, kb1 = 0xFu;
      if (keep) {
        const unsigned kw = keep[gp * 4 + (size_t)(oc >> 5)];  // oc and oc + 16 share the word
        kb0 = (kw >> (oc & 31)) & 0xFu;
        kb1 = (kw >> ((oc & 31) + 16)) & 0xFu;
      }
      f32x4 y0, y1;
      y0.x = fmaf(acc0[g][0], ldexpf(sv0.x, -ex), bv0.x);
      y0.y = fmaf(acc0[g][1], ldexpf(sv0.y, -ex), bv0.y);
      y0.z = fmaf(acc0[g][2], ldexpf(sv0.z, -ex), bv0.z);
      y0.w = fmaf(acc0[g][3], ldexpf(sv0.w, -ex), bv0.w);
      y1.x = fmaf(acc1[g][0], ldexpf(sv1.x, -ex), bv1.x);
      y1.y = fmaf(acc1[g][1], ldexpf(sv1.y, -ex), bv1.y);
      y1.z = fmaf(acc1[g][2], ldexpf(sv1.z, -ex), bv1.z);
      y1.w = fmaf(acc1[g][3], ldexpf(sv1.w, -ex), bv1.w);
      float* yp = y + gp * 128 + oc;
      __builtin_nontemporal_store(c7_act(y0, kb0, keep != nullptr, keep_scale, relu), reinterpret_cast<f32x4*>(yp));
      __builtin_nontemporal_store(c7_act(y1, kb1, keep != nullptr, keep_scale, relu), reinterpret_cast<f32x4*>(yp + 16));
    }
  }
}

// Weights [128 o][128 c][3][3] f32 (flip: use w[c][o][2-ky][2-kx], the input-gradient conv) -> the
// split A fragments of k_conv7_x3: GEMM row o, column k = tap * 128 + c (tap = 3 ky + kx), row
// scaled by 2^e_o (largest |w| of the row in [2^14, 2^15): k_conv_x3_pack's rule), hi = f16,
// lo = f16(x - hi); fragment order [chunk 36 = tap * 4 + c / 32][block 8 = o / 16][part 2 (hi, lo)]
// [k-group 4 = (c / 8) % 4][row 16 = o % 16][8 = c % 8]; inv[o] = 2^-e_o. One wave per row o.
__global__ __launch_bounds__(64) void k_conv7_pack(const float* __restrict__ wt, int flip, _Float16* __restrict__ out,
                                                   float* __restrict__ inv) {
  const int o = blockIdx.x, l = threadIdx.x;
  float a[18];
  float m = 0.0f;
#pragma unroll
  for (int j = 0; j < 18; ++j) {
    const int k = l + 64 * j, tap = k >> 7, c = k & 127;
    const int ky = tap / 3, kx = tap % 3;
    a[j] = flip ? wt[((c * 128 + o) * 3 + (2 - ky)) * 3 + (2 - kx)] : wt[((o * 128 + c) * 3 + ky) * 3 + kx];
    m = fmaxf(m, fabsf(a[j]));
  }
  m = wave_max_f(m);
  int e = 0;
  if (m > 0.0f && m < __builtin_inff()) {
    int fe;
    (void)frexpf(m, &fe);
    e = 15 - fe;
  }
  const int ob = o >> 4, row = o & 15;
#pragma unroll
  for (int j = 0; j < 18; ++j) {
    const int k = l + 64 * j, chunk = k >> 5, kg = (k >> 3) & 3, el = k & 7;
    const float s = ldexpf(a[j], e);
    const _Float16 hi = (_Float16)s;
    const _Float16 lo = (_Float16)(s - (float)hi);
    const size_t base = ((((size_t)chunk * 8 + ob) * 2) * 4 + kg) * 16 + row;  // part 0
    out[base * 8 + el] = hi;
    out[(base + 4 * 16) * 8 + el] = lo;
  }
  if (l == 0) inv[o] = ldexpf(1.0f, -e);
}

// ---- the weight gradient: dW[o][c][tap] = sum over boards b and pixels p of
// dz[b][p][o] * x[b][p + off(tap)][c] (zero padding): a GEMM of M = 128 (o) x N = 1152 (tap, c)
// over K = 49 B. k_conv_x3_wgrad's scheme with one board per step: the board's dz and x are
// scaled, split and stored pixel-major per channel ("transposed": the MFMA K is the pixel) in LDS
// with row stride 8 (7 columns + one zero column) — dz at k = 8 row + col (64 K-slots = 2 chunks
// of 32; row 7 and column 7 zero), x in a zero-haloed grid at 8 (row + 1) + col + 1, so tap
// (dy, dx) of slot k is x-grid element k + 8 dy + dx. The 576 output tiles of 16 x 16 are split
// over 4 workgroup roles (role r = output channels 32 r .. 32 r + 31, staged alone) x 8 waves
// (wave w = input channels 16 w ..) x 18 tiles (2 o-blocks x 9 taps); per K-chunk a wave reads 4
// A fragments (dz: 2 o-blocks, hi / lo) and per tap row two aligned B fragments from which
// dx = 0, 1, 2 are cut, then 54 MFMAs. Workgroup (bg, role) walks boards b = bg, += the number
// of board groups; the next board's loads are issued before this board's MFMAs. One running power
// of two per workgroup and operand, lowered (the accumulators rescaled, exactly) when a later
// board is larger. Partial sums in fragment order; k_conv7_wgrad_reduce adds them in a fixed order.
constexpr int kW7Threads = 512, kW7Waves = 8, kW7Roles = 4;
constexpr int kW7Groups = 64;                    // board groups (at most): 64 x 4 roles = one workgroup per CU
constexpr int kW7DyStride = 64 + 8;              // f16 per (channel, half): 36 dwords (4 x odd)
constexpr int kW7XStride = 88;                   // 9 grid rows + the fragment overreach: 44 dwords (4 x odd)
constexpr int kW7HalfDy = 32 * kW7DyStride, kW7HalfX = 128 * kW7XStride;
constexpr int kW7DyBytes = 2 * kW7HalfDy * 2, kW7XBytes = 2 * kW7HalfX * 2;
constexpr int kW7Tiles = 18;
constexpr int kW7DyItems = 7 * 4 * 8, kW7XItems = 7 * 4 * 32;  // (row, column pair, channel quad)
constexpr int kW7XIt = (kW7XItems + kW7Threads - 1) / kW7Threads;
constexpr int kW7Per = kW7Roles * kW7Waves * kW7Tiles * 64 * 4;  // floats per board group's partial (147456)
static_assert(kW7DyItems <= kW7Threads, "k_conv7_x3_wgrad: one dz item per thread");
static_assert(kW7Per == 128 * 1152, "k_conv7_x3_wgrad: partial size");

__device__ __forceinline__ int w7_exp(float m) {  // the scale exponent of a board maximum (1000: no constraint)
  if (!(m > 0.0f)) return 1000;
  return scale_exp(m);
}

__global__ __launch_bounds__(kW7Threads, 1) void k_conv7_x3_wgrad(const float* __restrict__ x,
                                                                  const float* __restrict__ dz, int B, int NBG,
                                                                  f32x4* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) _Float16 dyt[2 * kW7HalfDy];  // [half][32 o][kW7DyStride]
  __shared__ __attribute__((aligned(16))) _Float16 xt[2 * kW7HalfX];    // [half][128 c][kW7XStride]
  __shared__ float red[32];                                             // [parity][dz 8 | x 8] wave maxima
  const int tid = threadIdx.x, l = tid & 63, n = l & 15, ks = l >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int role = blockIdx.x & 3, bg = blockIdx.x >> 2;

  // zero both operands once: every board writes the same interior elements
  for (int i = tid; i < kW7DyBytes / 16; i += kW7Threads) reinterpret_cast<u32x4*>(dyt)[i] = u32x4{0u, 0u, 0u, 0u};
  for (int i = tid; i < kW7XBytes / 16; i += kW7Threads) reinterpret_cast<u32x4*>(xt)[i] = u32x4{0u, 0u, 0u, 0u};

  f32x4 acc[kW7Tiles];
#pragma unroll
  for (int t = 0; t < kW7Tiles; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  int E1 = 1000, E2 = 1000;  // the workgroup's operand exponents so far (1000: no data yet)

  const int a_base = n * kW7DyStride + 8 * ks;                // A: dz row o = 32 role + 16 j + n, k-group ks
  const int b_base = (16 * wave + n) * kW7XStride + 8 * ks;   // B: x row c = 16 wave + n

  const int nsteps = B > bg ? (B - 1 - bg) / NBG + 1 : 0;
  // board data in registers. dz item (row r, pair m, quad q): pixels (r, 2m), (r, 2m + 1) (column 7:
  // zero), channels 32 role + 4 q..; x item (row r, pair m, quad q): grid columns 2m, 2m + 1 = board
  // columns 2m - 1, 2m (column -1: zero), channels 4 q..
  f32x4 dv[2], xv[kW7XIt][2];
  const f32x4 zero4{0.f, 0.f, 0.f, 0.f};
  auto load = [&](int step) {
    const size_t b = (size_t)bg + (size_t)step * NBG;
    const f32x4* dzb = reinterpret_cast<const f32x4*>(dz + b * 6272);
    const f32x4* xb = reinterpret_cast<const f32x4*>(x + b * 6272);
    {
      const int q = tid & 7, m = (tid >> 3) & 3, r = tid >> 5;
      const bool ok = tid < kW7DyItems;
      const int p = r * 7 + 2 * m;
      dv[0] = ok ? __builtin_nontemporal_load(dzb + p * 32 + role * 8 + q) : zero4;
      dv[1] = ok && m < 3 ? __builtin_nontemporal_load(dzb + (p + 1) * 32 + role * 8 + q) : zero4;
    }
#pragma unroll
    for (int i = 0; i < kW7XIt; ++i) {
      const int it = tid + i * kW7Threads, q = it & 31, m = (it >> 5) & 3, r = it >> 7;
      const bool ok = it < kW7XItems;
      const int p = r * 7 + 2 * m;  // board pixel of grid column 2m + 1
      xv[i][0] = ok && m > 0 ? xb[(p - 1) * 32 + q] : zero4;
      xv[i][1] = ok ? xb[p * 32 + q] : zero4;
    }
  };
  if (nsteps > 0) load(0);

  for (int step = 0; step < nsteps; ++step) {
    const int par = step & 1;
    float my = max3_abs(max3_abs(0.0f, dv[0].x, dv[0].y), dv[0].z, dv[0].w);
    my = max3_abs(max3_abs(my, dv[1].x, dv[1].y), dv[1].z, dv[1].w);
    float mxx = 0.0f;
#pragma unroll
    for (int i = 0; i < kW7XIt; ++i)
#pragma unroll
      for (int h = 0; h < 2; ++h) mxx = max3_abs(max3_abs(mxx, xv[i][h].x, xv[i][h].y), xv[i][h].z, xv[i][h].w);
    my = wave_max_f(my);
    mxx = wave_max_f(mxx);
    if (l == 0) {  // parity-buffered: a slow wave may still read the last board's
      red[par * 16 + wave] = my;
      red[par * 16 + 8 + wave] = mxx;
    }
    __syncthreads();  // the previous board's MFMAs are done with the LDS (and the zeroing); the maxima are visible
    float ry = 0.0f, rx = 0.0f;
#pragma unroll
    for (int w = 0; w < kW7Waves; ++w) {
      ry = fmaxf(ry, red[par * 16 + w]);
      rx = fmaxf(rx, red[par * 16 + 8 + w]);
    }
    const int n1 = min(E1, w7_exp(ry)), n2 = min(E2, w7_exp(rx));
    if (E1 < 1000 && E2 < 1000 && n1 + n2 != E1 + E2) {  // larger values: rescale what is summed so far
      const float f = ldexpf(1.0f, (n1 + n2) - (E1 + E2));
#pragma unroll
      for (int t = 0; t < kW7Tiles; ++t) acc[t] = acc[t] * f;
    }
    E1 = n1;
    E2 = n2;
    const int s1 = E1 < 1000 ? E1 : 0, s2 = E2 < 1000 ? E2 : 0;
    // split and store pixel-major: a pair of pixels of one channel = one u32 per half
    if (tid < kW7DyItems) {
      const int q = tid & 7, m = (tid >> 3) & 3, r = tid >> 5;
      const float a0[4] = {dv[0].x, dv[0].y, dv[0].z, dv[0].w};
      const float a1[4] = {dv[1].x, dv[1].y, dv[1].z, dv[1].w};
      const int k = r * 8 + 2 * m;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        unsigned h, o;
        split2(ldexpf(a0[j], s1), ldexpf(a1[j], s1), h, o);
        const int ch = 4 * q + j;
        *reinterpret_cast<unsigned*>(dyt + ch * kW7DyStride + k) = h;
        *reinterpret_cast<unsigned*>(dyt + kW7HalfDy + ch * kW7DyStride + k) = o;
      }
    }
#pragma unroll
    for (int i = 0; i < kW7XIt; ++i) {
      const int it = tid + i * kW7Threads, q = it & 31, m = (it >> 5) & 3, r = it >> 7;
      if (it < kW7XItems) {
        const float a0[4] = {xv[i][0].x, xv[i][0].y, xv[i][0].z, xv[i][0].w};
        const float a1[4] = {xv[i][1].x, xv[i][1].y, xv[i][1].z, xv[i][1].w};
        const int k = (r + 1) * 8 + 2 * m;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          unsigned h, o;
          split2(ldexpf(a0[j], s2), ldexpf(a1[j], s2), h, o);
          const int ch = 4 * q + j;
          *reinterpret_cast<unsigned*>(xt + ch * kW7XStride + k) = h;
          *reinterpret_cast<unsigned*>(xt + kW7HalfX + ch * kW7XStride + k) = o;
        }
      }
    }
    if (step + 1 < nsteps) load(step + 1);  // the next board's loads, in flight under the MFMAs
    __syncthreads();
    // the board's 2 K-chunks of 32 pixel slots
#pragma unroll
    for (int kc = 0; kc < 2; ++kc) {
      const int k0 = 32 * kc;
      h16x8 ah[2], al[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        ah[j] = *reinterpret_cast<const h16x8*>(dyt + a_base + 16 * j * kW7DyStride + k0);
        al[j] = *reinterpret_cast<const h16x8*>(dyt + kW7HalfDy + a_base + 16 * j * kW7DyStride + k0);
      }
#pragma unroll
      for (int dr = 0; dr < 3; ++dr) {
        const int off = b_base + k0 + 8 * dr;
        const u32x4 h0 = *reinterpret_cast<const u32x4*>(xt + off), h1 = *reinterpret_cast<const u32x4*>(xt + off + 8);
        const u32x4 o0 = *reinterpret_cast<const u32x4*>(xt + kW7HalfX + off);
        const u32x4 o1 = *reinterpret_cast<const u32x4*>(xt + kW7HalfX + off + 8);
        h16x8 bh[3], bl[3];
        bh[0] = __builtin_bit_cast(h16x8, h0);
        bl[0] = __builtin_bit_cast(h16x8, o0);
        bh[1] = __builtin_bit_cast(h16x8, u32x4{__builtin_amdgcn_alignbit(h0.y, h0.x, 16), __builtin_amdgcn_alignbit(h0.z, h0.y, 16),
                                                __builtin_amdgcn_alignbit(h0.w, h0.z, 16), __builtin_amdgcn_alignbit(h1.x, h0.w, 16)});
        bl[1] = __builtin_bit_cast(h16x8, u32x4{__builtin_amdgcn_alignbit(o0.y, o0.x, 16), __builtin_amdgcn_alignbit(o0.z, o0.y, 16),
                                                __builtin_amdgcn_alignbit(o0.w, o0.z, 16), __builtin_amdgcn_alignbit(o1.x, o0.w, 16)});
        bh[2] = __builtin_bit_cast(h16x8, u32x4{h0.y, h0.z, h0.w, h1.x});
        bl[2] = __builtin_bit_cast(h16x8, u32x4{o0.y, o0.z, o0.w, o1.x});
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int dc = 0; dc < 3; ++dc) {
            f32x4& c = acc[j * 9 + dr * 3 + dc];
            asm volatile(
                "v_mfma_f32_16x16x32_f16 %0, %1, %2, %0\n\t"
                "v_mfma_f32_16x16x32_f16 %0, %3, %2, %0\n\t"
                "v_mfma_f32_16x16x32_f16 %0, %1, %4, %0"
                : "+a"(c)
                : "v"(ah[j]), "v"(bh[dc]), "v"(al[j]), "v"(bl[dc]));
          }
      }
    }
    ln_mfma_drain(acc);
  }
  // the partial sums, unscaled, in fragment order: part[bg][role][wave][tile][lane]
  const float u = (E1 < 1000 && E2 < 1000) ? ldexpf(1.0f, -(E1 + E2)) : 0.0f;
  f32x4* pb = part + (((size_t)bg * kW7Roles + role) * kW7Waves + wave) * kW7Tiles * 64 + l;
#pragma unroll
  for (int t = 0; t < kW7Tiles; ++t) pb[t * 64] = acc[t] * u;
}

// dW[o][c][ky][kx] (PyTorch's layout) = the sum over the G board groups' partials; one thread per
// (role, wave, tile, lane, element): 8 independent running sums (g mod 8) combined at the end (a
// fixed order: deterministic)
__global__ __launch_bounds__(256) void k_conv7_wgrad_reduce(const float* __restrict__ part, int G, float* __restrict__ dw) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= kW7Per) return;
  const int i = e & 3, l = (e >> 2) & 63, t = (e >> 8) % kW7Tiles, wr = (e >> 8) / kW7Tiles;
  const int wave = wr & 7, role = wr >> 3;
  const int o = 32 * role + 16 * (t / 9) + 4 * (l >> 4) + i, c = 16 * wave + (l & 15), tap = t % 9;
  float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  int g = 0;
  for (; g + 8 <= G; g += 8) {
#pragma unroll
    for (int j = 0; j < 8; ++j) s[j] += part[(size_t)(g + j) * kW7Per + e];
  }
  for (int j = 0; g < G; ++g, ++j) s[j] += part[(size_t)g * kW7Per + e];
  dw[(o * 128 + c) * 9 + tap] = ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]));
}

// ---- the first layer, 1 -> 128: y[b][p][o] = sum_tap w[o][tap] x[b][p + off(tap)] + bias[o] in
// fp32 (fmaf, taps in order 0..8), NHWC out, the same fused epilogue. One thread per (pixel,
// channel quad): a wave = 2 pixels x 128 channels, 512-B rows; the weights transposed in LDS.
__global__ __launch_bounds__(256) void k_conv7_first(const float* __restrict__ x, const float* __restrict__ w,
                                                     const float* __restrict__ bias, const unsigned* __restrict__ keep,
                                                     float keep_scale, int relu, float* __restrict__ y, long long npx) {
  __shared__ __attribute__((aligned(16))) float wt[10][128];  // [tap][o], row 9 = bias
  for (int i = threadIdx.x; i < 1152; i += 256) wt[i % 9][i / 9] = w[i];
  if (threadIdx.x < 128) wt[9][threadIdx.x] = bias ? bias[threadIdx.x] : 0.0f;
  __syncthreads();
  const int qq = threadIdx.x & 31, oc = 4 * qq;
  for (long long gp = (long long)blockIdx.x * 8 + (threadIdx.x >> 5); gp < npx; gp += (long long)gridDim.x * 8) {
    const long long b = gp / 49;
    const int pp = (int)(gp - b * 49), r = pp / 7, c = pp % 7;
    const float* xb = x + b * 49;
    f32x4 a{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int rr = r + t / 3 - 1, cc = c + t % 3 - 1;
      const float xv = (rr >= 0 && rr < 7 && cc >= 0 && cc < 7) ? xb[rr * 7 + cc] : 0.0f;
      const f32x4 wv = *reinterpret_cast<const f32x4*>(&wt[t][oc]);
      a.x = fmaf(wv.x, xv, a.x);
      a.y = fmaf(wv.y, xv, a.y);
      a.z = fmaf(wv.z, xv, a.z);
      a.w = fmaf(wv.w, xv, a.w);
    }
    const f32x4 bv = *reinterpret_cast<const f32x4*>(&wt[9][oc]);
    a = f32x4{a.x + bv.x, a.y + bv.y, a.z + bv.z, a.w + bv.w};
    unsigned kb = 0xFu;
    if (keep) kb = (keep[(size_t)gp * 4 + (size_t)(oc >> 5)] >> (oc & 31)) & 0xFu;
    *reinterpret_cast<f32x4*>(y + (size_t)gp * 128 + oc) = c7_act(a, kb, keep != nullptr, keep_scale, relu);
  }
}

// The first layer's weight gradient dW[o][tap] = sum over pixels of dz[b][p][o] x[b][p + off(tap)]:
// workgroup g sums a contiguous range of pixels (thread = (pixel parity, o): the even and the odd
// pixels of the range in order, then even + odd) into part[g][o][tap]; k_conv7_first_reduce adds the
// partials in a fixed order.
constexpr int kF7Grid = 1024;
__global__ __launch_bounds__(256) void k_conv7_first_wgrad(const float* __restrict__ x, const float* __restrict__ dz,
                                                           long long npx, long long per, float* __restrict__ part) {
  __shared__ float sh[128 * 9];
  const int o = threadIdx.x & 127, ph = threadIdx.x >> 7;
  const long long p0 = (long long)blockIdx.x * per, p1 = min(p0 + per, npx);
  float a[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (long long gp = p0 + ph; gp < p1; gp += 2) {
    const long long b = gp / 49;
    const int pp = (int)(gp - b * 49), r = pp / 7, c = pp % 7;
    const float* xb = x + b * 49;
    const float d = dz[(size_t)gp * 128 + o];
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int rr = r + t / 3 - 1, cc = c + t % 3 - 1;
      const float xv = (rr >= 0 && rr < 7 && cc >= 0 && cc < 7) ? xb[rr * 7 + cc] : 0.0f;
      a[t] = fmaf(d, xv, a[t]);
    }
  }
  if (ph == 1) {
#pragma unroll
    for (int t = 0; t < 9; ++t) sh[o * 9 + t] = a[t];
  }
  __syncthreads();
  if (ph == 0) {
#pragma unroll
    for (int t = 0; t < 9; ++t) part[(size_t)blockIdx.x * 1152 + o * 9 + t] = a[t] + sh[o * 9 + t];
  }
}

__global__ __launch_bounds__(128) void k_conv7_first_reduce(const float* __restrict__ part, int G, float* __restrict__ dw) {
  const int e = blockIdx.x * 128 + threadIdx.x;
  if (e >= 1152) return;
  float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  int g = 0;
  for (; g + 8 <= G; g += 8) {
#pragma unroll
    for (int j = 0; j < 8; ++j) s[j] += part[(size_t)(g + j) * 1152 + e];
  }
  for (int j = 0; g < G; ++g, ++j) s[j] += part[(size_t)g * 1152 + e];
  dw[e] = ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]));
}

// ---- the dropout's keep bits: 4 x u32 per pixel, bit c of the 128 = channel c kept. Generator:
// Philox-4x32-10 (Salmon et al., SC'11) with key = the two 32-bit halves of key[0] and counter =
// (the two halves of the element index e, the two halves of key[1]); e = (4 pixel + word) * 8 + j
// gives the random words of channels 32 word + 4 j .. + 3; a channel is kept when its word is
// >= round(p 2^32) (p = 0: always). No state, no host synchronisation: the key is read on the device.
__device__ __forceinline__ void philox4x32_10(unsigned (&c)[4], unsigned k0, unsigned k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned hi0 = __umulhi(0xD2511F53u, c[0]), lo0 = 0xD2511F53u * c[0];
    const unsigned hi1 = __umulhi(0xCD9E8D57u, c[2]), lo1 = 0xCD9E8D57u * c[2];
    const unsigned n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
    c[0] = n0;
    c[1] = lo1;
    c[2] = n2;
    c[3] = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
}

__global__ __launch_bounds__(256) void k_dropout_keep(const unsigned long long* __restrict__ key, long long nwords,
                                                      unsigned thr, unsigned* __restrict__ keep) {
  const unsigned long long k0 = key[0], k1 = key[1];
  for (long long wi = (long long)blockIdx.x * 256 + threadIdx.x; wi < nwords; wi += (long long)gridDim.x * 256) {
    unsigned bits = 0u;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const unsigned long long e = (unsigned long long)wi * 8ull + (unsigned long long)j;
      unsigned c[4] = {(unsigned)e, (unsigned)(e >> 32), (unsigned)k1, (unsigned)(k1 >> 32)};
      philox4x32_10(c, (unsigned)k0, (unsigned)(k0 >> 32));
#pragma unroll
      for (int i = 0; i < 4; ++i) bits |= (c[i] >= thr ? 1u : 0u) << (4 * j + i);
    }
    keep[wi] = bits;
  }
}

// dz = gy * [y > 0] * keep_scale: relu(dropout(z)) = y and y > 0 implies kept, so the backward of
// the fused Dropout -> ReLU needs the saved output only. One streaming float4 pass.
__global__ __launch_bounds__(256) void k_conv7_act_grad(const f32x4* __restrict__ gy, const f32x4* __restrict__ y,
                                                        long long n4, float keep_scale, f32x4* __restrict__ dz) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
    const f32x4 g = __builtin_nontemporal_load(gy + i), v = __builtin_nontemporal_load(y + i);
    f32x4 r;
    r.x = v.x > 0.0f ? g.x * keep_scale : 0.0f;
    r.y = v.y > 0.0f ? g.y * keep_scale : 0.0f;
    r.z = v.z > 0.0f ? g.z * keep_scale : 0.0f;
    r.w = v.w > 0.0f ? g.w * keep_scale : 0.0f;
    __builtin_nontemporal_store(r, dz + i);
  }
}

__host__ inline bool a16(const void* p) { return ((uintptr_t)p & 15u) == 0; }
__host__ inline int stream_grid(long long items, int per_block, int cap) {
  const long long g = (items + per_block - 1) / per_block;
  return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}

}  // namespace
}  // namespace bk

using namespace bk;

extern "C" {

int bk_conv7_tile_boards(void) { return kC7T; }

int bk_conv7_weight_bytes(void) { return kC7WBytes; }

int bk_conv7_pack(const float* w, int flip, void* wsplit, float* inv, void* stream) {
  BK_REQUIRE(w && wsplit && inv, "bad argument");
  BK_REQUIRE(a16(wsplit) && a16(inv), "bk_conv7_pack: 16-byte aligned outputs");
  hipLaunchKernelGGL(k_conv7_pack, dim3(128), dim3(64), 0, (hipStream_t)stream, w, flip, (_Float16*)wsplit, inv);
  return launch_check("k_conv7_pack");
}

int bk_conv7(const float* x, int B, const void* wsplit, const float* inv, const float* bias, const uint32_t* keep,
             float keep_scale, int relu, float* y, void* stream) {
  BK_REQUIRE(x && wsplit && inv && y && B >= 0, "bad argument");
  BK_REQUIRE(a16(x) && a16(wsplit) && a16(inv) && a16(y) && (!bias || a16(bias)) && (!keep || a16(keep)),
             "bk_conv7: 16-byte aligned buffers");
  if (B == 0) return BK_OK;
  {
    const void* fns[1] = {(const void*)k_conv7_x3};
    if (set_max_dynamic_lds(fns, 1, kC7Lds) != BK_OK) return BK_EHIP;
  }
  const int ntiles = (B + kC7T - 1) / kC7T;
  const int G = ntiles < 256 ? ntiles : 256;  // persistent: one workgroup per CU, tiles strided
  hipLaunchKernelGGL(k_conv7_x3, dim3(G), dim3(kLnThreads), kC7Lds, (hipStream_t)stream, x, (const h16x8*)wsplit, inv,
                     bias, keep, keep_scale, relu, y, B);
  return launch_check("k_conv7_x3");
}

int bk_conv7_wgrad_workspace_floats(int B) {
  const int G = B < kW7Groups ? (B > 0 ? B : 1) : kW7Groups;
  return G * kW7Per;
}

int bk_conv7_wgrad(const float* x, const float* dz, int B, float* workspace, float* dw, void* stream) {
  BK_REQUIRE(dw && B >= 0 && (B == 0 || (x && dz && workspace)), "bad argument");
  BK_REQUIRE(a16(x) && a16(dz) && a16(workspace), "bk_conv7_wgrad: 16-byte aligned buffers");
  hipStream_t s = (hipStream_t)stream;
  if (B == 0) return hipMemsetAsync(dw, 0, 128 * 128 * 9 * sizeof(float), s) == hipSuccess ? BK_OK : BK_EHIP;
  const int G = B < kW7Groups ? B : kW7Groups;
  hipLaunchKernelGGL(k_conv7_x3_wgrad, dim3(G * kW7Roles), dim3(kW7Threads), 0, s, x, dz, B, G, (f32x4*)workspace);
  if (launch_check("k_conv7_x3_wgrad") != BK_OK) return BK_EHIP;
  hipLaunchKernelGGL(k_conv7_wgrad_reduce, dim3((kW7Per + 255) / 256), dim3(256), 0, s, workspace, G, dw);
  return launch_check("k_conv7_wgrad_reduce");
}

int bk_conv7_first(const float* x, int B, const float* w, const float* bias, const uint32_t* keep, float keep_scale,
                   int relu, float* y, void* stream) {
  BK_REQUIRE(x && w && y && B >= 0, "bad argument");
  BK_REQUIRE(a16(y) && (!keep || a16(keep)), "bk_conv7_first: 16-byte aligned buffers");
  if (B == 0) return BK_OK;
  const long long npx = (long long)B * 49;
  hipLaunchKernelGGL(k_conv7_first, dim3(stream_grid(npx, 8, 256 * 16)), dim3(256), 0, (hipStream_t)stream, x, w, bias,
                     keep, keep_scale, relu, y, npx);
  return launch_check("k_conv7_first");
}

int bk_conv7_first_wgrad(const float* x, const float* dz, int B, float* workspace, float* dw, void* stream) {
  BK_REQUIRE(dw && B >= 0 && (B == 0 || (x && dz && workspace)), "bad argument");
  BK_REQUIRE(a16(dz) && a16(workspace), "bk_conv7_first_wgrad: 16-byte aligned buffers");
  hipStream_t s = (hipStream_t)stream;
  if (B == 0) return hipMemsetAsync(dw, 0, 128 * 9 * sizeof(float), s) == hipSuccess ? BK_OK : BK_EHIP;
  // at most min(B, 64) * 128 workgroups of >= 1 pixel each: within bk_conv7_wgrad_workspace_floats(B)
  const long long npx = (long long)B * 49;
  const int gmax = (B < kW7Groups ? B : kW7Groups) * 128;
  const int G = stream_grid(npx, 64, gmax < kF7Grid ? gmax : kF7Grid);
  const long long per = (npx + G - 1) / G;
  hipLaunchKernelGGL(k_conv7_first_wgrad, dim3(G), dim3(256), 0, s, x, dz, npx, per, workspace);
  if (launch_check("k_conv7_first_wgrad") != BK_OK) return BK_EHIP;
  hipLaunchKernelGGL(k_conv7_first_reduce, dim3(9), dim3(128), 0, s, workspace, G, dw);
  return launch_check("k_conv7_first_reduce");
}

int bk_dropout_keep(const int64_t* key, int64_t n_pixels, float p, uint32_t* keep, void* stream) {
  BK_REQUIRE(key && n_pixels >= 0 && (n_pixels == 0 || keep) && p >= 0.0f && p <= 1.0f, "bad argument");
  BK_REQUIRE(a16(keep) && ((uintptr_t)key & 7u) == 0, "bk_dropout_keep: aligned buffers");
  if (n_pixels == 0) return BK_OK;
  const double t = (double)p * 4294967296.0 + 0.5;
  const unsigned thr = t >= 4294967295.0 ? 0xFFFFFFFFu : (unsigned)t;
  const long long nwords = n_pixels * 4;
  hipLaunchKernelGGL(k_dropout_keep, dim3(stream_grid(nwords, 256, 256 * 32)), dim3(256), 0, (hipStream_t)stream,
                     (const unsigned long long*)key, nwords, thr, keep);
  return launch_check("k_dropout_keep");
}

int bk_conv7_act_grad(const float* gy, const float* y, int64_t n, float keep_scale, float* dz, void* stream) {
  BK_REQUIRE(n >= 0 && n % 4 == 0 && (n == 0 || (gy && y && dz)), "bad argument");
  BK_REQUIRE(a16(gy) && a16(y) && a16(dz), "bk_conv7_act_grad: 16-byte aligned buffers");
  if (n == 0) return BK_OK;
  hipLaunchKernelGGL(k_conv7_act_grad, dim3(stream_grid(n / 4, 256, 256 * 32)), dim3(256), 0, (hipStream_t)stream,
                     (const f32x4*)gy, (const f32x4*)y, n / 4, keep_scale, (f32x4*)dz);
  return launch_check("k_conv7_act_grad");
}

}  // extern "C"

// conv128.hip — DCNNet's convolutions for the leaf evaluator (nets.LeafDCNNet): the 128 -> 128
// 3x3 pad-1 layers at 14x14 and 20x20 on split-f16 MFMA products (k_conv7_x3's scheme and
// arithmetic, ppoconv.hip, on another tile geometry; 7x7 is k_conv7_x3 itself), and the first
// layer (2P input planes -> 128) in plain fp32, from the planar observation (k_conv128_first) or
// from the packed states themselves (k_conv128_first_states, the same bits). Activations are NHWC
// f32 [B][N][N][128].
//
// k_conv128_x3<N>: persistent, one workgroup of 4 waves per CU walking tiles of T boards (N = 14:
// 2 boards = 392 pixels, N = 20: 1 board = 400 pixels; 25 MFMA column groups of 16 either way, so
// k_conv7_x3's register budget holds: 2 x 25 accumulators = 200 AGPRs, 100 VGPRs of staging). The
// tile's boards share one zero-haloed LDS grid per plane with the odd row stride N + 1 slots of
// 16 B: row 0 zero, then per board N rows and one zero row; column 0 zero, and the right halo of
// a row is column 0 of the next one (the slot after the last row's end is the plane's one slot of
// overreach). 22 x 21 + 1 slots (N = 20) or 31 x 15 + 1 (N = 14, two boards) per plane, 16 planes
// = 116 / 120 KB. The pixel -> MFMA column map is C7PixMap's greedy (16 slots distinct mod 16 per
// group where the classes allow). Weights: bk_conv7_pack's fragments (they do not depend on the
// board size). Every board has its own power-of-two scale, so a board's output depends neither on
// its batch nor on its place in the tile.
// Epilogue: y = acc * inv[o] * 2^-ex(board) + bias[o], then (optional) ReLU; NHWC store.
#include "../../include/blokus_engine.h"
#include "ctx.h"

#include "leafnet_common.h"

namespace bk {
namespace {

template <int N_>
struct C128Geom {
  static constexpr int N = N_, NN = N * N;
  static constexpr int T = N == 14 ? 2 : 1;           // boards per tile
  static constexpr int RS = N + 1;                    // grid row stride in slots (odd)
  static constexpr int Rows = 1 + T * (N + 1);        // grid rows
  static constexpr int Px = NN * T;                   // pixels per tile
  static constexpr int NG = 25;                       // MFMA column groups
  static constexpr int PL = ((Rows * RS + 1) * 16 + 255) / 256 * 256;  // plane bytes (+ 1 slot: the last halo)
  static constexpr int Lds = 16 * PL + 128;           // 16 planes + board maxima [8] + board exponents [8]
  static_assert(N == 14 || N == 20, "k_conv128_x3: 14x14 or 20x20");
  static_assert(RS % 2 == 1, "k_conv128_x3: odd row stride (balanced slot classes mod 16)");
  static_assert(NG % kLnSlots == 0 && NG * 16 >= Px, "k_conv128_x3: groups");
  static_assert(T <= 8, "k_conv128_x3: board maxima");
  static_assert(Lds <= 160 * 1024, "k_conv128_x3: LDS");
  __host__ __device__ static constexpr int slot(int p) {  // tile pixel -> grid slot
    return (1 + (p / NN) * (N + 1) + (p % NN) / N) * RS + (p % NN) % N + 1;
  }
  __device__ static __forceinline__ int pixel(int sl) {  // grid slot -> tile pixel
    const int r1 = sl / RS - 1, col = sl % RS - 1;
    return (r1 / (N + 1)) * NN + (r1 % (N + 1)) * N + col;
  }
};
// the furthest read: the last pixel's slot + one row + one column, + 16 B, inside the plane
static_assert((C128Geom<20>::slot(C128Geom<20>::Px - 1) + C128Geom<20>::RS + 2) * 16 <= C128Geom<20>::PL, "N = 20");
static_assert((C128Geom<14>::slot(C128Geom<14>::Px - 1) + C128Geom<14>::RS + 2) * 16 <= C128Geom<14>::PL, "N = 14");

constexpr int kC128Chunks = 36;
constexpr int kC128WBytes = kC128Chunks * 8 * 2 * kBlock * 2;  // bk_conv7_weight_bytes()
constexpr int kC128Flip = 6;                                   // k_conv7_x3's kC7Flip (the same sums)

// C7PixMap's greedy on the geometry's grid; -1 = spare column
template <class G>
struct C128PixMap {
  int slot[G::NG * 16];
  constexpr C128PixMap() : slot() {
    bool used[G::Px] = {};
    for (int i = 0; i < G::NG * 16; ++i) slot[i] = -1;
    for (int g = 0; g < G::NG; ++g)
      for (int r = 0; r < 16; ++r)
        for (int p = 0; p < G::Px; ++p) {
          const int sl = G::slot(p);
          if (!used[p] && sl % 16 == r) {
            used[p] = true;
            slot[g * 16 + r] = sl;
            break;
          }
        }
    int p = 0;
    for (int i = 0; i < G::NG * 16; ++i) {
      if (slot[i] >= 0) continue;
      while (p < G::Px && used[p]) ++p;
      if (p == G::Px) break;
      used[p] = true;
      slot[i] = G::slot(p);
    }
  }
};
template <class G>
__device__ constexpr C128PixMap<G> kC128PixMap{};

// c7_chunk (ppoconv.hip): one K chunk for two output blocks that share the B fragments
template <int NG, int HALF>
__device__ __forceinline__ void c128_chunk(f32x4 (&acc0)[NG], f32x4 (&acc1)[NG], h16x8 a0h, h16x8 a0l, h16x8 a1h,
                                           h16x8 a1l, const unsigned char* grid, const int (&pb)[NG], int coff,
                                           int coff_next, h16x8 (&rb)[kLnSlots][2]) {
  static_assert(NG % kLnSlots == 0, "c128_chunk: the ring slot of a group must not depend on the chunk");
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

__device__ __forceinline__ f32x4 c128_act(f32x4 v, int relu) {
  if (relu) {
    v.x = max_bits(v.x, 0);
    v.y = max_bits(v.y, 0);
    v.z = max_bits(v.z, 0);
    v.w = max_bits(v.w, 0);
  }
  return v;
}

template <int N>
__global__ __launch_bounds__(kLnThreads, 1) void k_conv128_x3(const float* __restrict__ x,
                                                              const h16x8* __restrict__ w,
                                                              const float* __restrict__ inv,
                                                              const float* __restrict__ bias, int relu,
                                                              float* __restrict__ y, int B) {
  using G = C128Geom<N>;
  constexpr int RS = G::RS, NG = G::NG, PL = G::PL, NN = G::NN, T = G::T, Px = G::Px;
  constexpr int HQ = Px * 16;                                // float4 quads per channel half of a tile
  constexpr int HIT = (HQ + kLnThreads - 1) / kLnThreads;    // 25
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  unsigned char* act = lds;  // 16 planes [hi | lo][grid slots][16 B] of the staged channel half
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
    const int sl = kC128PixMap<G>.slot[16 * g + n];
    ab[g] = (sl >= 0 ? sl : RS + 1) * 16 + ks * 4 * PL - kBias;
    valid |= (sl >= 0 ? 1u : 0u) << g;
  }
  const __amdgpu_buffer_rsrc_t wrs = ln_rsrc(w, (unsigned)kC128WBytes);
  auto wload = [&](int chunk, int j, int part) {
    return __builtin_bit_cast(
        h16x8, __builtin_amdgcn_raw_buffer_load_b128(wrs, l * 16, ((chunk * 8 + 2 * wave + j) * 2 + part) * 1024, 0));
  };
  // (negated: the accumulators end up holding the negated sums, kC128Flip)
  const f32x4 sv0 = -*reinterpret_cast<const f32x4*>(inv + oc), sv1 = -*reinterpret_cast<const f32x4*>(inv + oc + 16);
  const f32x4 zero4{0.f, 0.f, 0.f, 0.f};
  const f32x4 bv0 = bias ? *reinterpret_cast<const f32x4*>(bias + oc) : zero4;
  const f32x4 bv1 = bias ? *reinterpret_cast<const f32x4*>(bias + oc + 16) : zero4;
  auto coff_of = [&](int c) {  // chunk c of a half: tap c / 2, quarter c % 2 of the half
    const int t = c >> 1;
    return 2 * (c & 1) * PL + ((t / 3 - 1) * RS + (t % 3 - 1)) * 16 + kBias;
  };

  const int ntiles = (B + T - 1) / T;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const size_t px0 = (size_t)tile * Px;  // the tile's first pixel
    const int npx = min(Px, (B - tile * T) * NN);
    // channel half 0 of the tile into registers (item i = quad tid + 256 i) and, in the same pass,
    // the per-board maxima over both halves (half 1 is read again, from the L2, when it is staged);
    // a wave's 64 quads are 4 consecutive pixels, in at most two boards
    // (the thread and wave ids pass through empty asm statements per tile: the per-item addresses
    // are then computed where they are used instead of being hoisted out of the tile loop)
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
      float m = max3_abs(max3_abs(0.0f, xv[i].x, xv[i].y), xv[i].z, xv[i].w);
      m = max3_abs(max3_abs(m, x1.x, x1.y), x1.z, x1.w);
      if (T == 1) {
        const float m0 = wave_max_f(m);
        if (l == 0) atomicMax(&bmax[0], __builtin_bit_cast(unsigned, m0));
      } else {
        const int p_lo = (wv * 64 + i * kLnThreads) >> 4;
        const int bd = min(p / NN, T - 1), bd_lo = min(p_lo / NN, T - 1), bd_hi = min((p_lo + 3) / NN, T - 1);
        const float m_lo = wave_max_f(bd == bd_lo ? m : 0.0f);
        if (l == 0) atomicMax(&bmax[bd_lo], __builtin_bit_cast(unsigned, m_lo));
        if (bd_hi != bd_lo) {  // wave-uniform
          const float m_hi = wave_max_f(bd == bd_hi ? m : 0.0f);
          if (l == 0) atomicMax(&bmax[bd_hi], __builtin_bit_cast(unsigned, m_hi));
        }
      }
    }
    __syncthreads();  // the maxima are complete; every wave is done with the previous tile
    if (tid < T) {
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
          const int ex = bex[T == 1 ? 0 : p / NN];
          unsigned h0, h1, l0, l1;
          split2(ldexpf(v.x, ex), ldexpf(v.y, ex), h0, l0);
          split2(ldexpf(v.z, ex), ldexpf(v.w, ex), h1, l1);
          unsigned char* d = act + ((o & 3) * 4 + (o >> 2) * 2) * PL + G::slot(p) * 16 + (qq & 1) * 8;
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
        if (c == kC128Flip && h == 1) {  // from here on the accumulators hold the negated sums (kC7Flip)
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
        const unsigned sgn = (h == 1 && c >= kC128Flip) ? 0x80008000u : 0u;
        h16x8 wc[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const u32x4 u = __builtin_bit_cast(u32x4, wq[c & 1][j]);
          wc[j] = __builtin_bit_cast(h16x8, u32x4{u.x ^ sgn, u.y ^ sgn, u.z ^ sgn, u.w ^ sgn});
        }
        c128_chunk<NG, PL>(acc0, acc1, wc[0], wc[1], wc[2], wc[3], act, ab, coff_of(c),
                           coff_of(c + 1 < 18 ? c + 1 : c), rb);
      }
    }
    ln_mfma_drain(acc0);
    ln_mfma_drain(acc1);

    // y = acc * inv * 2^-ex(board) + bias (ReLU), NHWC
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      if (!((valid >> g) & 1u)) continue;
      int sb = ab[g];
      asm volatile("" : "+v"(sb));  // as above: the pixel of column g is computed here, per tile
      const int p = G::pixel((sb - ks * 4 * PL + kBias) / 16);
      if (p >= npx) continue;
      const int ex = bex[T == 1 ? 0 : p / NN];
      const size_t gp = px0 + (size_t)p;
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
      __builtin_nontemporal_store(c128_act(y0, relu), reinterpret_cast<f32x4*>(yp));
      __builtin_nontemporal_store(c128_act(y1, relu), reinterpret_cast<f32x4*>(yp + 16));
    }
  }
}

// ---- the first layer, CIN (4 / 6 / 8 observation planes) -> 128: y[b][p][o] = sum over taps t
// (outer, 0..8) and input channels c (inner) of w[o][c][t] x[b][c][p + off(t)] + bias[o] in fp32
// (fmaf in that order), then (optional) ReLU. x planar [B][CIN][N][N] as the search writes it, y
// NHWC. A workgroup step takes 32 consecutive pixels: their 9 CIN input values (zero padding
// applied) go to LDS once, then a thread computes a channel quad of 4 of the pixels (local pixels
// sub + 8 j: every weight quad read from LDS serves all four; a wave stores 2 x 512-B rows per
// j). The weights sit transposed in LDS, [k = tap * CIN + c][o].
constexpr int kC128FirstPx = 4;
template <int CIN>
__global__ __launch_bounds__(256) void k_conv128_first(const float* __restrict__ x, const float* __restrict__ w,
                                                       const float* __restrict__ bias, int relu,
                                                       float* __restrict__ y, int N, long long npx) {
  constexpr int K = 9 * CIN, KP = (K + 3) / 4 * 4, J = kC128FirstPx, PXB = 8 * J;
  __shared__ __attribute__((aligned(16))) float wt[K + 1][128];  // last row = bias
  __shared__ __attribute__((aligned(16))) float xs[PXB][KP];     // [local pixel][k] (k >= K: unused)
  const int NN = N * N;
  for (int i = threadIdx.x; i < 128 * K; i += 256) {
    const int o = i / K, r = i - o * K, c = r / 9, t = r - c * 9;  // w[o][c][t]
    wt[t * CIN + c][o] = w[i];
  }
  if (threadIdx.x < 128) wt[K][threadIdx.x] = bias ? bias[threadIdx.x] : 0.0f;
  for (int i = threadIdx.x; i < PXB * KP; i += 256) (&xs[0][0])[i] = 0.0f;
  const int qq = threadIdx.x & 31, oc = 4 * qq, sub = threadIdx.x >> 5;
  for (long long base = (long long)blockIdx.x * PXB; base < npx; base += (long long)gridDim.x * PXB) {
    __syncthreads();  // the weights (first step); the previous step's reads of xs
    for (int i = threadIdx.x; i < PXB * K; i += 256) {
      const int lp = i / K, k = i - lp * K, t = k / CIN, ci = k - t * CIN;
      const long long gp = base + lp;
      float v = 0.0f;
      if (gp < npx) {
        const long long b = gp / NN;
        const int pp = (int)(gp - b * NN), r = pp / N, c = pp - r * N;
        const int rr = r + t / 3 - 1, cc = c + t % 3 - 1;
        if (rr >= 0 && rr < N && cc >= 0 && cc < N) v = x[(b * CIN + ci) * NN + rr * N + cc];
      }
      xs[lp][k] = v;
    }
    __syncthreads();
    f32x4 a[J];
#pragma unroll
    for (int j = 0; j < J; ++j) a[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
    for (int k4 = 0; k4 < KP / 4; ++k4) {
      f32x4 xq[J];
#pragma unroll
      for (int j = 0; j < J; ++j) xq[j] = *reinterpret_cast<const f32x4*>(&xs[sub + 8 * j][4 * k4]);
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        if (4 * k4 + kk < K) {
          const f32x4 wv = *reinterpret_cast<const f32x4*>(&wt[4 * k4 + kk][oc]);
#pragma unroll
          for (int j = 0; j < J; ++j) {
            const float xv = xq[j][kk];
            a[j].x = fmaf(wv.x, xv, a[j].x);
            a[j].y = fmaf(wv.y, xv, a[j].y);
            a[j].z = fmaf(wv.z, xv, a[j].z);
            a[j].w = fmaf(wv.w, xv, a[j].w);
          }
        }
      }
    }
    const f32x4 bv = *reinterpret_cast<const f32x4*>(&wt[K][oc]);
#pragma unroll
    for (int j = 0; j < J; ++j) {
      const long long gp = base + sub + 8 * j;
      if (gp >= npx) continue;
      const f32x4 v = f32x4{a[j].x + bv.x, a[j].y + bv.y, a[j].z + bv.z, a[j].w + bv.w};
      *reinterpret_cast<f32x4*>(y + (size_t)gp * 128 + oc) = c128_act(v, relu);
    }
  }
}

// ---- the first layer from packed states: k_conv128_first's sums on the observation planes of
// states [B][kStateWords] (k_observe, env.hip: plane c < P at (r, col) = bit col of word c kMaxN + r,
// plane P + q = all ones iff q == the to-move word) without the planes. The inputs are 0 or 1 and
// fmaf(w, 1, a) = a + w, fmaf(w, 0, a) = a for finite w (a is never -0: it starts at +0), so the
// terms of zero inputs are left out and the bits equal k_conv128_first's. A wave takes one board
// row at a time (items strided over all waves): its 3 P row words, shifted up one bit so that bit 0
// and the bits from N + 1 are the zero halo, and the to-move word sit in scalar registers; a lane
// owns two output channels, whose 9 P piece weights and the 9 weights of the to-move plane it keeps
// in registers (from a transposed LDS copy), so a pixel costs 9 packed fmas for the to-move
// plane, P more for each occupied tap, and one 512-byte row of the NHWC store per wave.
// (Shifts: the words hold bits 0..N + 1 <= 21; the furthest one read is N - 1 + 2 + 3 <= 24.)
constexpr int kC128StatesPx = 4;
// bit `pos` of a (wave-uniform) word as 0.0f or 1.0f
__device__ __forceinline__ float bit_one(uint32_t word, int pos) {
  return __builtin_bit_cast(float, ((word >> pos) & 1u) * 0x3f800000u);
}
template <int P>
__global__ __launch_bounds__(256) void k_conv128_first_states(const uint32_t* __restrict__ states,
                                                              const int32_t* __restrict__ status,
                                                              const float* __restrict__ w,
                                                              const float* __restrict__ bias, int relu,
                                                              float* __restrict__ y, int N, int B) {
  constexpr int CIN = 2 * P, K = 9 * CIN, NIT = K / 2, RSW = 130;
  // the weights transposed, [r = c * 9 + tap][o], last row = bias; row stride 130: a wave's writes
  // (consecutive r) step two banks. Every thread's NIT loads are in flight before the first write.
  __shared__ __attribute__((aligned(16))) float wt[K + 1][RSW];
  {
    float tmp[NIT];
#pragma unroll
    for (int it = 0; it < NIT; ++it) tmp[it] = w[it * 256 + threadIdx.x];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int i = it * 256 + threadIdx.x, o = i / K, r = i - o * K;  // w[o][c][t] = w[o][r]
      wt[r][o] = tmp[it];
    }
  }
  if (threadIdx.x < 128) wt[K][threadIdx.x] = bias ? bias[threadIdx.x] : 0.0f;
  __syncthreads();
  const int oc = 2 * (threadIdx.x & 63);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  f32x2 wp[9][P];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int c = 0; c < P; ++c) wp[t][c] = *reinterpret_cast<const f32x2*>(&wt[c * 9 + t][oc]);
  const f32x2 bv = *reinterpret_cast<const f32x2*>(&wt[K][oc]);
  const uint32_t rowmask = ((1u << N) - 1u) << 1;
  const int nitems = B * N;
  for (int item = blockIdx.x * 4 + wave; item < nitems; item += gridDim.x * 4) {
    const int b = item / N, r = item - b * N;
    uint32_t rw[3][P], occ[3], inb[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      occ[d] = inb[d] = 0u;
#pragma unroll
      for (int c = 0; c < P; ++c) rw[d][c] = 0u;
    }
    int tm = -1;
    if (!status || status[b] == 1) {  // (wave-uniform) other rows: the all-zero observation, no state read
      const uint32_t* s = states + (size_t)b * kStateWords;
      tm = (int)s[kWToMove];
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        const int rr = r + d - 1;
        if (rr < 0 || rr >= N) continue;
#pragma unroll
        for (int c = 0; c < P; ++c) {
          rw[d][c] = (s[c * kMaxN + rr] << 1) & rowmask;
          occ[d] |= rw[d][c];
        }
        inb[d] = rowmask;
      }
    }
    const bool has_tm = tm >= 0 && tm < P;
    f32x2 wm[9];
#pragma unroll
    for (int t = 0; t < 9; ++t)
      wm[t] = has_tm ? *reinterpret_cast<const f32x2*>(&wt[(P + tm) * 9 + t][oc]) : f32x2{0.f, 0.f};
    if (!has_tm) inb[0] = inb[1] = inb[2] = 0u;
    float* yrow = y + (size_t)item * N * 128 + oc;
    // kC128StatesPx pixels at a time: their fma chains are independent (each one in
    // k_conv128_first's order), so they overlap; a tap's piece planes are skipped when none of the
    // pixels has a piece there. The columns past N - 1 of the last step read halo bits (zeros) and
    // are not stored.
    for (int col = 0; col < N; col += kC128StatesPx) {
      f32x2 a[kC128StatesPx];
#pragma unroll
      for (int j = 0; j < kC128StatesPx; ++j) a[j] = f32x2{0.f, 0.f};
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const int d = t / 3, sh = col + t % 3;
        constexpr uint32_t kPxMask = (1u << kC128StatesPx) - 1u;
        if ((occ[d] >> sh) & kPxMask) {
#pragma unroll
          for (int c = 0; c < P; ++c) {
            if (!((rw[d][c] >> sh) & kPxMask)) continue;  // (wave-uniform) this plane is empty under all the pixels
#pragma unroll
            for (int j = 0; j < kC128StatesPx; ++j) {
              const float xv = bit_one(rw[d][c], sh + j);
              a[j].x = fmaf(wp[t][c].x, xv, a[j].x);
              a[j].y = fmaf(wp[t][c].y, xv, a[j].y);
            }
          }
        }
        if (((inb[d] >> sh) & kPxMask) == kPxMask) {  // (wave-uniform) the tap is on the board for all the pixels
#pragma unroll
          for (int j = 0; j < kC128StatesPx; ++j) a[j] = pk_add(a[j], wm[t]);  // = fmaf(w, 1, a)
        } else {
#pragma unroll
          for (int j = 0; j < kC128StatesPx; ++j) {
            const float xm = bit_one(inb[d], sh + j);
            a[j].x = fmaf(wm[t].x, xm, a[j].x);
            a[j].y = fmaf(wm[t].y, xm, a[j].y);
          }
        }
      }
#pragma unroll
      for (int j = 0; j < kC128StatesPx; ++j) {
        if (col + j >= N) break;
        f32x2 v{a[j].x + bv.x, a[j].y + bv.y};
        if (relu) {
          v.x = max_bits(v.x, 0);
          v.y = max_bits(v.y, 0);
        }
        *reinterpret_cast<f32x2*>(yrow + (size_t)(col + j) * 128) = v;
      }
    }
  }
}

__host__ inline bool a16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

template <int N>
int launch_conv128(const float* x, int B, const void* wsplit, const float* inv, const float* bias, int relu, float* y,
                   hipStream_t s) {
  using G = C128Geom<N>;
  {
    const void* fns[1] = {(const void*)k_conv128_x3<N>};
    if (set_max_dynamic_lds(fns, 1, G::Lds) != BK_OK) return BK_EHIP;
  }
  const int ntiles = (B + G::T - 1) / G::T;
  const int grid = ntiles < 256 ? ntiles : 256;  // persistent: one workgroup per CU, tiles strided
  hipLaunchKernelGGL(k_conv128_x3<N>, dim3(grid), dim3(kLnThreads), G::Lds, s, x, (const h16x8*)wsplit, inv, bias,
                     relu, y, B);
  return launch_check("k_conv128_x3");
}

}  // namespace
}  // namespace bk

using namespace bk;

extern "C" {

int bk_conv128_x3_supported(int N) { return N == 7 || N == 14 || N == 20; }

int bk_conv128_x3_tile_boards(int N) {
  return N == 7 ? bk_conv7_tile_boards() : N == 14 ? C128Geom<14>::T : N == 20 ? C128Geom<20>::T : 0;
}

int bk_conv128_x3(const float* x, int B, int N, const void* wsplit, const float* inv, const float* bias, int relu,
                  float* y, void* stream) {
  BK_REQUIRE(wsplit && inv && B >= 0 && (B == 0 || (x && y)), "bad argument");  // (an empty batch has no buffers)
  BK_REQUIRE(bk_conv128_x3_supported(N), "bk_conv128_x3: board size must be 7, 14 or 20");
  BK_REQUIRE(a16(x) && a16(wsplit) && a16(inv) && a16(y) && (!bias || a16(bias)),
             "bk_conv128_x3: 16-byte aligned buffers");
  if (B == 0) return BK_OK;
  if (N == 7) return bk_conv7(x, B, wsplit, inv, bias, nullptr, 1.0f, relu, y, stream);
  if (N == 14) return launch_conv128<14>(x, B, wsplit, inv, bias, relu, y, (hipStream_t)stream);
  return launch_conv128<20>(x, B, wsplit, inv, bias, relu, y, (hipStream_t)stream);
}

int bk_conv128_first(const float* obs, int B, int N, int cin, const float* w, const float* bias, int relu, float* y,
                     void* stream) {
  BK_REQUIRE(w && B >= 0 && (B == 0 || (obs && y)), "bad argument");
  BK_REQUIRE(N == 7 || N == 14 || N == 20, "bk_conv128_first: board size must be 7, 14 or 20");
  BK_REQUIRE(cin == 4 || cin == 6 || cin == 8, "bk_conv128_first: 4, 6 or 8 input planes");
  BK_REQUIRE(a16(y), "bk_conv128_first: 16-byte aligned output");
  if (B == 0) return BK_OK;
  const long long npx = (long long)B * N * N;
  const long long per = 8 * kC128FirstPx, g = (npx + per - 1) / per;
  const dim3 grid((unsigned)(g > 768 ? 768 : g));  // 3 resident workgroups per CU, each transposing the weights once
  hipStream_t s = (hipStream_t)stream;
  if (cin == 4)
    hipLaunchKernelGGL(k_conv128_first<4>, grid, dim3(256), 0, s, obs, w, bias, relu, y, N, npx);
  else if (cin == 6)
    hipLaunchKernelGGL(k_conv128_first<6>, grid, dim3(256), 0, s, obs, w, bias, relu, y, N, npx);
  else
    hipLaunchKernelGGL(k_conv128_first<8>, grid, dim3(256), 0, s, obs, w, bias, relu, y, N, npx);
  return launch_check("k_conv128_first");
}

int bk_conv128_first_states(const void* states, const int32_t* status, int B, int N, int P, const float* w,
                            const float* bias, int relu, float* y, void* stream) {
  BK_REQUIRE(w && B >= 0 && (B == 0 || (states && y)), "bad argument");
  BK_REQUIRE(N == 7 || N == 14 || N == 20, "bk_conv128_first_states: board size must be 7, 14 or 20");
  BK_REQUIRE(P >= 2 && P <= 4, "bk_conv128_first_states: 2, 3 or 4 players");
  BK_REQUIRE(a16(y) && ((uintptr_t)states & 3u) == 0, "bk_conv128_first_states: aligned buffers");
  BK_REQUIRE((long long)B * N <= 0x7fff0000LL, "bk_conv128_first_states: batch too large");
  if (B == 0) return BK_OK;
  const int items = B * N, g = (items + 3) / 4;  // one board row per wave and step
  const dim3 grid((unsigned)(g > 1024 ? 1024 : g));  // 4 resident workgroups per CU, each transposing the weights once
  hipStream_t s = (hipStream_t)stream;
  const uint32_t* st = (const uint32_t*)states;
  if (P == 2)
    hipLaunchKernelGGL(k_conv128_first_states<2>, grid, dim3(256), 0, s, st, status, w, bias, relu, y, N, B);
  else if (P == 3)
    hipLaunchKernelGGL(k_conv128_first_states<3>, grid, dim3(256), 0, s, st, status, w, bias, relu, y, N, B);
  else
    hipLaunchKernelGGL(k_conv128_first_states<4>, grid, dim3(256), 0, s, st, status, w, bias, relu, y, N, B);
  return launch_check("k_conv128_first_states");
}

}  // extern "C"

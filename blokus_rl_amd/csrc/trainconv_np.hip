// trainconv_np.hip — the learner's 3x3 convolutions 64 -> 64 on 7x7 and 14x14 boards: trainconv.hip's
// split-f16 MFMA arithmetic (three f16 products per fp32 product, the ln_chunk / ln_chunk_il K loop
// over 18 chunks = 9 taps x 2 halves of 32 input channels) on the tilings the small boards need.
// The weight fragments and row scales are bk_conv_x3_pack's (flip included).
//
// k_conv_x3_np<N>: forward (y = conv(x) + b) and input gradient (the same kernel on the flipped /
// transposed weights). Persistent, one workgroup of 4 waves per CU (wave w = output channels
// 16w..16w+15) walking tiles (tile = blockIdx.x, += gridDim.x; the last tile may be partial); the
// next tile's NHWC input is loaded into registers under the current tile's MFMAs.
//   14x14: one board per tile, the zero-haloed grid of leafnet_common.h (16 rows x 18 slots of
//          16 B per plane; 196 pixels = 12.25 MFMA groups, padded to 15).
//   7x7:   one board is 49 pixels = 4 MFMA groups, too little per A fragment streamed from L2, so a
//          tile is a column of 8 boards (ppoconv.hip's c7_slot grid): 65 rows x 9 slots per plane
//          — row 0 zero, then per board 7 rows and one zero row shared with the next board, columns
//          0 and 8 zero; 392 pixels = 24.5 groups, padded to 25. With 64 channels the 16 planes
//          (8 octets x hi / lo) hold the whole K: one staging per tile.
// Every board has its own power-of-two input scale (largest magnitude into [2^14, 2^15)), applied
// when the board is staged and removed in the epilogue by the board of the accumulator's column;
// an MFMA column depends on its own B column only and the K order is the same in every column, so
// a board's output is bitwise a function of that board and the weights alone: its tile neighbours,
// its place in the tile and the batch size do not enter.
//
// k_conv_x3_np_wgrad<N> + k_conv_x3_np_wgrad_reduce: dW[o][c][tap] = sum over boards b and pixels
// p of dy[b][p][o] * x[b][p + off(tap)][c]; k_conv_x3_wgrad's scheme (the MFMA K is the pixel; 8
// waves, wave w = input channels 16 (w % 4).., output channels 32 (w / 4).., 18 accumulator tiles;
// per K-chunk 4 A fragments and per tap row two aligned B fragments from which dx = 0, 1, 2 are
// cut) with the K tiling chosen per board size, one trip = whole boards:
//   7x7:   4 boards per trip, each 8 rows (7 + a zero row, shared as the x grid's separator) x 8
//          columns (7 + a zero column): K = 256 pixel slots = 8 chunks of 32.
//   14x14: 1 board per trip as 14 rows x 16 columns: K = 224 = 7 chunks.
// dy sits at k = row * CS + col, x in a zero-haloed grid at (row + 1) * CS + col + 1, so tap
// (dr, dc) of slot k is x-grid element k + CS dr + dc. One power-of-two scale per workgroup and
// operand, lowered (the accumulators rescaled, exactly) when a later trip holds larger values; the
// partial sums go to a workspace in fragment order and are added in a fixed order (deterministic).
//
// The sign-flip trick of ppoconv.hip (kC7Flip) is not used here. The f16 MFMA's one-signed
// accumulation bias (about -0.07 of the rms error) matters only where many kernel outputs are
// summed in fp32 afterwards. K = 576 as in k_conv_x3, which runs without the flip; the forward's
// outputs go into the batch norm's fp64 statistics, where a bias of 1e-8 relative is three orders
// below the 5e-6 bar of the fused conv + BN; the bias gradients are sums of dy, not of this
// kernel's outputs; and the weight gradient's sum over pixels is the accumulator itself: its
// 36864 outputs are not summed any further. All checks are per element.
#include "../../include/blokus_engine.h"
#include "ctx.h"

#include "leafnet_common.h"

#ifndef BK_CONV_NP_IL
#define BK_CONV_NP_IL 1  // k_conv_x3_np: ln_chunk_il (the B-fragment reads between the MFMAs)
#endif

namespace bk {
namespace {

// ---- forward / input gradient
template <int N>
struct NcGeo {
  static_assert(N == 7 || N == 14, "k_conv_x3_np: 7x7 and 14x14 boards");
  static constexpr int T = N == 7 ? 8 : 1;        // boards per tile
  static constexpr int BP = N * N;                // pixels per board
  static constexpr int PX = T * BP;               // pixels per tile
  static constexpr int RS = N == 7 ? 9 : ln_row(14);  // grid row stride in slots (9: odd, 18: ln_row's)
  static constexpr int ROWS = 1 + T * (N + 1);    // zero row, then per board N rows + a zero row
  static constexpr int NG = ((PX + 15) / 16 + kLnSlots - 1) / kLnSlots * kLnSlots;
  static constexpr int PL = (ROWS * RS * 16 + 255) / 256 * 256;  // plane bytes
  static constexpr int LDS = 16 * PL + 128;       // 16 planes + board maxima [8] + board exponents [8]
  static constexpr int slot(int p) {              // tile pixel -> grid slot
    return (1 + (p / BP) * (N + 1) + (p % BP) / N) * RS + (p % BP) % N + 1;
  }
  static constexpr int pixel(int sl) {            // grid slot -> tile pixel
    const int r1 = sl / RS - 1, col = sl % RS - 1;
    return (r1 / (N + 1)) * BP + (r1 % (N + 1)) * N + col;
  }
};
static_assert(NcGeo<7>::LDS == 151680 && NcGeo<7>::LDS <= 160 * 1024, "k_conv_x3_np<7>: LDS");
static_assert(NcGeo<14>::LDS == 73856 && NcGeo<14>::LDS <= 160 * 1024, "k_conv_x3_np<14>: LDS");
static_assert(NcGeo<7>::T <= 8 && NcGeo<14>::T <= 8, "k_conv_x3_np: the board maxima hold 8 boards");
static_assert(NcGeo<14>::NG == ln_groups(14) && NcGeo<14>::PL == ln_plane(14), "k_conv_x3_np<14>: leafnet_common.h's grid");

// LnPixMap's greedy on the tile's grid: each group takes one pixel per slot class mod 16 where the
// classes allow (conflict-free B-fragment reads), leftovers fill the gaps; -1 = spare column.
template <int N>
struct NcPixMap {
  using G = NcGeo<N>;
  int slot[G::NG * 16];
  constexpr NcPixMap() : slot() {
    bool used[G::PX] = {};
    for (int i = 0; i < G::NG * 16; ++i) slot[i] = -1;
    for (int g = 0; g < G::NG; ++g)
      for (int r = 0; r < 16; ++r)
        for (int p = 0; p < G::PX; ++p) {
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
      while (p < G::PX && used[p]) ++p;
      if (p == G::PX) break;
      used[p] = true;
      slot[i] = G::slot(p);
    }
  }
  // every tile pixel in exactly one column, every other column spare, slot <-> pixel consistent
  constexpr bool bijection() const {
    bool seen[G::PX] = {};
    int spare = 0;
    for (int i = 0; i < G::NG * 16; ++i) {
      if (slot[i] < 0) {
        ++spare;
        continue;
      }
      const int p = G::pixel(slot[i]);
      if (p < 0 || p >= G::PX || seen[p] || G::slot(p) != slot[i]) return false;
      seen[p] = true;
    }
    return spare == G::NG * 16 - G::PX;
  }
};
template <int N>
__device__ constexpr NcPixMap<N> kNcPixMap{};
static_assert(NcPixMap<7>{}.bijection(), "k_conv_x3_np<7>: the pixel map is a bijection onto the tile");
static_assert(NcPixMap<14>{}.bijection(), "k_conv_x3_np<14>: the pixel map is a bijection onto the tile");

template <int N>
__global__ __launch_bounds__(kLnThreads, 1) void k_conv_x3_np(const float* __restrict__ x, const h16x8* __restrict__ w,
                                                              const float* __restrict__ inv,
                                                              const float* __restrict__ bias, float* __restrict__ y,
                                                              int B) {
  using G = NcGeo<N>;
  constexpr int T = G::T, BP = G::BP, PX = G::PX, RS = G::RS, NG = G::NG, PL = G::PL;
  constexpr int QN = PX * 16, QIT = (QN + kLnThreads - 1) / kLnThreads;  // float4 quads of the tile
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  unsigned char* act = lds;  // 16 planes [hi q | lo q][ROWS x RS slots][16 B]
  unsigned* bmax = reinterpret_cast<unsigned*>(lds + 16 * PL);  // [8] board maxima (float bits)
  int* bex = reinterpret_cast<int*>(lds + 16 * PL + 32);        // [8] board exponents
  const int tid = threadIdx.x, l = tid & 63, n = l & 15, ks = l >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int oc = 16 * wave + 4 * ks;
  const f32x4 zero4{0.f, 0.f, 0.f, 0.f};

  // a tile's input into registers (issued one tile ahead: its HBM latency under the MFMAs); with 64
  // channels quad q of the tile is float4 q of its dense NHWC buffer
  const int ntiles = (B + T - 1) / T;
  f32x4 xv[QIT];
  auto load = [&](int tile) {
    const f32x4* xt = reinterpret_cast<const f32x4*>(x + (size_t)tile * PX * 64);
    const int nq = min(PX, (B - tile * T) * BP) * 16;
#pragma unroll
    for (int i = 0; i < QIT; ++i) {
      const int q = tid + i * kLnThreads;
      xv[i] = q < nq ? __builtin_nontemporal_load(xt + q) : zero4;
    }
  };
  int tile = blockIdx.x;
  if (tile < ntiles) load(tile);
  // zero the grid once: every tile writes the interiors only (absent boards as zeros)
  for (int i = tid; i < 16 * PL / 16; i += kLnThreads) reinterpret_cast<u32x4*>(lds)[i] = u32x4{0u, 0u, 0u, 0u};
  if (tid < 8) bmax[tid] = 0u;
  __syncthreads();

  constexpr int kBias = (RS + 1) * 16;
  int ab[NG];
  unsigned valid = 0;
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    const int sl = kNcPixMap<N>.slot[16 * g + n];
    ab[g] = (sl >= 0 ? sl : RS + 1) * 16 + ks * 4 * PL - kBias;
    valid |= (sl >= 0 ? 1u : 0u) << g;
  }
  const __amdgpu_buffer_rsrc_t wrs = ln_rsrc(w, 18u * 8u * 1024u);
  auto wload = [&](int c, int p) {
    return __builtin_bit_cast(h16x8, __builtin_amdgcn_raw_buffer_load_b128(wrs, l * 16, ((c * 8 + wave * 2 + p) * 64) * 16, 0));
  };
  const f32x4 sv = *reinterpret_cast<const f32x4*>(inv + oc);
  const f32x4 bv = bias ? *reinterpret_cast<const f32x4*>(bias + oc) : zero4;
  auto coff_of = [&](int c) {
    const int t = c >> 1;
    return 2 * (c & 1) * PL + ((t / 3 - 1) * RS + (t % 3 - 1)) * 16 + kBias;
  };

  for (; tile < ntiles; tile += gridDim.x) {
    const size_t px0 = (size_t)tile * PX;  // the tile's first pixel
    const int npx = min(PX, (B - tile * T) * BP);
    h16x8 wq[kLnWpf + 1][2];
#pragma unroll
    for (int c = 0; c < kLnWpf; ++c) {
      wq[c][0] = wload(c, 0);
      wq[c][1] = wload(c, 1);
    }
    // (the thread and wave ids pass through empty asm statements per tile: the per-item slots are
    // then computed where they are used instead of being hoisted out of the tile loop and held in
    // registers across the MFMA phase)
    int t0 = tid, wv = wave;
    asm volatile("" : "+v"(t0), "+s"(wv));
    // the per-board maxima: a wave's 64 quads of an item are 4 consecutive pixels, in at most two boards
#pragma unroll
    for (int i = 0; i < QIT; ++i) {
      const float m = max3_abs(max3_abs(0.0f, xv[i].x, xv[i].y), xv[i].z, xv[i].w);
      if (T == 1) {
        const float mw = wave_max_f(m);
        if (l == 0) atomicMax(&bmax[0], __builtin_bit_cast(unsigned, mw));
      } else {
        const int p = (t0 + i * kLnThreads) >> 4, p_lo = (wv * 64 + i * kLnThreads) >> 4;
        const int bd = min(p / BP, T - 1), bd_lo = min(p_lo / BP, T - 1), bd_hi = min((p_lo + 3) / BP, T - 1);
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
    // scale by the board's power of two, split, into the planes: quad qq of pixel p = channels
    // 4qq..4qq+3, octet o = qq / 2 (hi plane 4 (o % 4) + 2 (o / 4), lo the next), half qq % 2
#pragma unroll
    for (int i = 0; i < QIT; ++i) {
      const int q = t0 + i * kLnThreads, p = q >> 4, qq = q & 15, o = qq >> 1;
      if (q < QN) {
        const int ex = bex[T == 1 ? 0 : p / BP];
        unsigned h0, h1, l0, l1;
        split2(ldexpf(xv[i].x, ex), ldexpf(xv[i].y, ex), h0, l0);
        split2(ldexpf(xv[i].z, ex), ldexpf(xv[i].w, ex), h1, l1);
        unsigned char* d = act + ((o & 3) * 4 + (o >> 2) * 2) * PL + G::slot(p) * 16 + (qq & 1) * 8;
        *reinterpret_cast<u32x2*>(d) = u32x2{h0, h1};
        *reinterpret_cast<u32x2*>(d + PL) = u32x2{l0, l1};
      }
    }
    if (tile + (int)gridDim.x < ntiles) load(tile + gridDim.x);  // the next tile, in flight under this one's MFMAs
    __syncthreads();

    // the 18 chunks (tap c/2, channel half c%2), weights kLnWpf chunks ahead
    f32x4 acc[NG];
    h16x8 rb[kLnSlots][2];
    ln_prime<NG, PL>(rb, act, ab, coff_of(0));
#pragma unroll
    for (int c = 0; c < 18; ++c) {
      const int cn = c + kLnWpf, sn = cn % (kLnWpf + 1);
      if (cn < 18) {
        wq[sn][0] = wload(cn, 0);
        wq[sn][1] = wload(cn, 1);
      }
      const h16x8* wc = wq[c % (kLnWpf + 1)];
#if BK_CONV_NP_IL
      if (c == 0)
        ln_chunk_il<NG, true, PL>(acc, wc[0], wc[1], act, ab, coff_of(0), coff_of(1), rb);
      else
        ln_chunk_il<NG, false, PL>(acc, wc[0], wc[1], act, ab, coff_of(c), coff_of(c + 1 < 18 ? c + 1 : c), rb);
#else
      if (c == 0)
        ln_chunk<NG, true, PL>(acc, wc[0], wc[1], act, ab, coff_of(0), coff_of(1), rb);
      else
        ln_chunk<NG, false, PL>(acc, wc[0], wc[1], act, ab, coff_of(c), coff_of(c + 1 < 18 ? c + 1 : c), rb);
#endif
    }
#if BK_CONV_NP_IL
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the last chunk's untracked read-ahead
#endif
    ln_mfma_drain(acc);

    // y = acc * inv * 2^-ex(board) + bias, NHWC
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      if (!((valid >> g) & 1u)) continue;
      int sb = ab[g];
      asm volatile("" : "+v"(sb));  // as above: the pixel of column g is computed here, per tile
      const int p = G::pixel((sb - ks * 4 * PL + kBias) / 16);
      if (p >= npx) continue;
      const int ex = bex[T == 1 ? 0 : p / BP];
      const f32x2 s01{ldexpf(sv.x, -ex), ldexpf(sv.y, -ex)}, s23{ldexpf(sv.z, -ex), ldexpf(sv.w, -ex)};
      const f32x2 y01 = pk_fma(f32x2{acc[g][0], acc[g][1]}, s01, f32x2{bv.x, bv.y});
      const f32x2 y23 = pk_fma(f32x2{acc[g][2], acc[g][3]}, s23, f32x2{bv.z, bv.w});
      __builtin_nontemporal_store(f32x4{y01.x, y01.y, y23.x, y23.y},
                                  reinterpret_cast<f32x4*>(y + (px0 + (size_t)p) * 64 + oc));
    }
  }
}

// ---- the weight gradient
constexpr int kNwThreads = 512, kNwWaves = 8;
constexpr int kNwGrid = 256;   // workgroups (at most): one per CU
constexpr int kNwTiles = 18;   // (o-block of the wave's pair, tap) tiles per wave
constexpr int kNwPer = kNwWaves * kNwTiles * 64 * 4;  // floats per workgroup partial (36864)
static_assert(kNwPer == 64 * 64 * 9, "k_conv_x3_np_wgrad: partial size");

template <int N>
struct NwGeo {
  static_assert(N == 7 || N == 14, "k_conv_x3_np_wgrad: 7x7 and 14x14 boards");
  static constexpr int T = N == 7 ? 4 : 1;     // boards per trip
  static constexpr int CS = N == 7 ? 8 : 16;   // column stride: N columns + zero columns
  static constexpr int RB = N == 7 ? 8 : 14;   // rows per board (7x7: + the zero row between boards)
  static constexpr int KS = T * RB * CS;       // K slots per trip (256, 224)
  static constexpr int DyStride = KS + 8;               // f16 per (channel, half)
  static constexpr int XStride = KS + 8 + 2 * CS;       // + two tap rows and the fragment overreach
  static constexpr int HalfDy = 64 * DyStride, HalfX = 64 * XStride;
  static constexpr int DyBytes = 2 * HalfDy * 2, XBytes = 2 * HalfX * 2;
  static constexpr int LDS = DyBytes + XBytes + 128;
  static constexpr int MPd = (N + 1) / 2, MPx = N / 2 + 1;  // column pairs per row: dy (cols 2m, 2m+1), x (2m-1, 2m)
  static constexpr int DyItems = T * N * MPd * 16, XItems = T * N * MPx * 16;  // (board, row, pair, channel quad)
  static constexpr int DyIt = (DyItems + kNwThreads - 1) / kNwThreads, XIt = (XItems + kNwThreads - 1) / kNwThreads;
  static_assert(KS % 32 == 0, "whole K-chunks");
  static_assert((DyStride / 2) % 4 == 0 && ((DyStride / 8) & 1) == 1, "dy rows: 4 x odd dwords (conflict-free reads)");
  static_assert((XStride / 2) % 4 == 0 && ((XStride / 8) & 1) == 1, "x rows: 4 x odd dwords (conflict-free reads)");
  static_assert(XStride >= (T * RB + 2) * CS, "the x grid with its zero rows");
  // the last B fragment: chunk KS - 32, k-group 3, tap row 2, 16 elements (both aligned halves)
  static_assert(KS - 32 + 24 + 2 * CS + 16 <= XStride && KS - 32 + 24 + 8 <= DyStride, "fragment reads in bounds");
  static_assert(LDS <= 160 * 1024, "k_conv_x3_np_wgrad: LDS");
};

__device__ __forceinline__ int nw_exp(float m) {  // the scale exponent of a trip maximum (1000: no constraint)
  if (!(m > 0.0f)) return 1000;
  return scale_exp(m);
}

template <int N>
__global__ __launch_bounds__(kNwThreads, 1) void k_conv_x3_np_wgrad(const float* __restrict__ x,
                                                                    const float* __restrict__ dy, int B,
                                                                    f32x4* __restrict__ part) {
  using G = NwGeo<N>;
  constexpr int NN = N * N, T = G::T, CS = G::CS, RB = G::RB;
  constexpr int kDyStride = G::DyStride, kXStride = G::XStride, kHalfDy = G::HalfDy, kHalfX = G::HalfX;
  constexpr int kDyIt = G::DyIt, kXIt = G::XIt;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  _Float16* dyt = reinterpret_cast<_Float16*>(lds);                      // [half][64 o][DyStride]
  _Float16* xt = reinterpret_cast<_Float16*>(lds + G::DyBytes);          // [half][64 c][XStride]
  float* red = reinterpret_cast<float*>(lds + G::DyBytes + G::XBytes);   // [parity][dy 8 | x 8] wave maxima
  const int tid = threadIdx.x, l = tid & 63, n = l & 15, ks = l >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int cb = wave & 3, oh = wave >> 2;
  const f32x4 zero4{0.f, 0.f, 0.f, 0.f};

  // zero both operands once: every trip writes the same interior elements (absent boards as zeros)
  for (int i = tid; i < (G::DyBytes + G::XBytes) / 16; i += kNwThreads)
    reinterpret_cast<u32x4*>(lds)[i] = u32x4{0u, 0u, 0u, 0u};

  f32x4 acc[kNwTiles];
#pragma unroll
  for (int t = 0; t < kNwTiles; ++t) acc[t] = zero4;
  int E1 = 1000, E2 = 1000;  // the workgroup's operand exponents so far (1000: no data yet)

  const int a_base = (32 * oh + n) * kDyStride + 8 * ks;  // A: dy row o = 32 oh + 16 j + n, k-group ks
  const int b_base = (16 * cb + n) * kXStride + 8 * ks;   // B: x row c = 16 cb + n

  const int ntrips = (B + T - 1) / T;
  const int nsteps = ntrips > (int)blockIdx.x ? (ntrips - 1 - (int)blockIdx.x) / (int)gridDim.x + 1 : 0;
  // trip data in registers. dy item (board j, row r, pair m, quad q): pixels (r, 2m), (r, 2m + 1)
  // (column N: zero); x item: grid columns 2m, 2m + 1 = board columns 2m - 1, 2m (outside: zero)
  f32x4 dv[kDyIt][2], xv[kXIt][2];
  auto load = [&](int step) {
    const int b0 = ((int)blockIdx.x + step * (int)gridDim.x) * T;
    int t0 = tid;
    asm volatile("" : "+v"(t0));  // the item addresses are computed here, not held across the MFMA phase
#pragma unroll
    for (int i = 0; i < kDyIt; ++i) {
      const int it = t0 + i * kNwThreads, q = it & 15, m = (it >> 4) % G::MPd, rr = (it >> 4) / G::MPd;
      const int j = rr / N, r = rr % N;
      const bool ok = it < G::DyItems && b0 + j < B;
      const f32x4* src = reinterpret_cast<const f32x4*>(dy + ((size_t)(b0 + j) * NN + r * N + 2 * m) * 64) + q;
      dv[i][0] = ok ? __builtin_nontemporal_load(src) : zero4;
      dv[i][1] = ok && 2 * m + 1 < N ? __builtin_nontemporal_load(src + 16) : zero4;
    }
#pragma unroll
    for (int i = 0; i < kXIt; ++i) {
      const int it = t0 + i * kNwThreads, q = it & 15, m = (it >> 4) % G::MPx, rr = (it >> 4) / G::MPx;
      const int j = rr / N, r = rr % N, c0 = 2 * m - 1;
      const bool ok = it < G::XItems && b0 + j < B;
      const f32x4* src = reinterpret_cast<const f32x4*>(x + ((size_t)(b0 + j) * NN + r * N) * 64) + q;
      xv[i][0] = ok && c0 >= 0 ? src[c0 * 16] : zero4;
      xv[i][1] = ok && c0 + 1 < N ? src[(c0 + 1) * 16] : zero4;
    }
  };
  if (nsteps > 0) load(0);

  for (int step = 0; step < nsteps; ++step) {
    const int par = step & 1;
    int t0 = tid;
    asm volatile("" : "+v"(t0));
    float my = 0.0f, mxx = 0.0f;
#pragma unroll
    for (int i = 0; i < kDyIt; ++i)
#pragma unroll
      for (int h = 0; h < 2; ++h) my = max3_abs(max3_abs(my, dv[i][h].x, dv[i][h].y), dv[i][h].z, dv[i][h].w);
#pragma unroll
    for (int i = 0; i < kXIt; ++i)
#pragma unroll
      for (int h = 0; h < 2; ++h) mxx = max3_abs(max3_abs(mxx, xv[i][h].x, xv[i][h].y), xv[i][h].z, xv[i][h].w);
    my = wave_max_f(my);
    mxx = wave_max_f(mxx);
    if (l == 0) {  // parity-buffered [par][dy 8 | x 8]: a slow wave may still read the last trip's
      red[par * 16 + wave] = my;
      red[par * 16 + 8 + wave] = mxx;
    }
    __syncthreads();  // the previous trip's MFMAs are done with the LDS (and the zeroing); the maxima are visible
    float ry = 0.0f, rx = 0.0f;
#pragma unroll
    for (int w = 0; w < kNwWaves; ++w) {
      ry = fmaxf(ry, red[par * 16 + w]);
      rx = fmaxf(rx, red[par * 16 + 8 + w]);
    }
    const int n1 = min(E1, nw_exp(ry)), n2 = min(E2, nw_exp(rx));
    if (E1 < 1000 && E2 < 1000 && n1 + n2 != E1 + E2) {  // larger values: rescale what is summed so far
      const float f = ldexpf(1.0f, (n1 + n2) - (E1 + E2));
#pragma unroll
      for (int t = 0; t < kNwTiles; ++t) acc[t] = acc[t] * f;
    }
    E1 = n1;
    E2 = n2;
    const int s1 = E1 < 1000 ? E1 : 0, s2 = E2 < 1000 ? E2 : 0;
    // split and store pixel-major: a pair of pixels of one channel = one u32 per half
#pragma unroll
    for (int i = 0; i < kDyIt; ++i) {
      const int it = t0 + i * kNwThreads, q = it & 15, m = (it >> 4) % G::MPd, rr = (it >> 4) / G::MPd;
      if (it < G::DyItems) {
        const float a0[4] = {dv[i][0].x, dv[i][0].y, dv[i][0].z, dv[i][0].w};
        const float a1[4] = {dv[i][1].x, dv[i][1].y, dv[i][1].z, dv[i][1].w};
        const int k = ((rr / N) * RB + rr % N) * CS + 2 * m;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          unsigned h, o;
          split2(ldexpf(a0[j], s1), ldexpf(a1[j], s1), h, o);
          const int ch = 4 * q + j;
          *reinterpret_cast<unsigned*>(dyt + ch * kDyStride + k) = h;
          *reinterpret_cast<unsigned*>(dyt + kHalfDy + ch * kDyStride + k) = o;
        }
      }
    }
#pragma unroll
    for (int i = 0; i < kXIt; ++i) {
      const int it = t0 + i * kNwThreads, q = it & 15, m = (it >> 4) % G::MPx, rr = (it >> 4) / G::MPx;
      if (it < G::XItems) {
        const float a0[4] = {xv[i][0].x, xv[i][0].y, xv[i][0].z, xv[i][0].w};
        const float a1[4] = {xv[i][1].x, xv[i][1].y, xv[i][1].z, xv[i][1].w};
        const int k = ((rr / N) * RB + rr % N + 1) * CS + 2 * m;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          unsigned h, o;
          split2(ldexpf(a0[j], s2), ldexpf(a1[j], s2), h, o);
          const int ch = 4 * q + j;
          *reinterpret_cast<unsigned*>(xt + ch * kXStride + k) = h;
          *reinterpret_cast<unsigned*>(xt + kHalfX + ch * kXStride + k) = o;
        }
      }
    }
    if (step + 1 < nsteps) load(step + 1);  // the next trip's loads, in flight under the MFMAs
    __syncthreads();
    // the trip's K-chunks of 32 pixel slots
#pragma unroll 1
    for (int kc = 0; kc < G::KS / 32; ++kc) {
      const int k0 = 32 * kc;
      h16x8 ah[2], al[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        ah[j] = *reinterpret_cast<const h16x8*>(dyt + a_base + 16 * j * kDyStride + k0);
        al[j] = *reinterpret_cast<const h16x8*>(dyt + kHalfDy + a_base + 16 * j * kDyStride + k0);
      }
#pragma unroll
      for (int dr = 0; dr < 3; ++dr) {
        const int off = b_base + k0 + CS * dr;
        const u32x4 h0 = *reinterpret_cast<const u32x4*>(xt + off), h1 = *reinterpret_cast<const u32x4*>(xt + off + 8);
        const u32x4 o0 = *reinterpret_cast<const u32x4*>(xt + kHalfX + off);
        const u32x4 o1 = *reinterpret_cast<const u32x4*>(xt + kHalfX + off + 8);
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
            f32x4& c = acc[j * 9 + dr * 3 + dc];  // hi*hi, lo*hi, hi*lo: k_conv_x3_wgrad's order
            c = mfma16(ah[j], bh[dc], c);
            c = mfma16(al[j], bh[dc], c);
            c = mfma16(ah[j], bl[dc], c);
          }
      }
    }
  }
  // the partial sums, unscaled, in fragment order: part[block][wave][tile][lane]
  const float u = (E1 < 1000 && E2 < 1000) ? ldexpf(1.0f, -(E1 + E2)) : 0.0f;
  f32x4* pb = part + ((size_t)blockIdx.x * kNwWaves + wave) * kNwTiles * 64 + l;
#pragma unroll
  for (int t = 0; t < kNwTiles; ++t) pb[t * 64] = acc[t] * u;
}

// dW[o][c][ky][kx] (PyTorch's layout) = the sum over the G workgroups' partials; one thread per
// (wave, tile, lane, element): 8 independent running sums (g mod 8) combined at the end (a
// fixed order: deterministic)
__global__ __launch_bounds__(256) void k_conv_x3_np_wgrad_reduce(const float* __restrict__ part, int G,
                                                                 float* __restrict__ dw) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= kNwPer) return;
  const int i = e & 3, l = (e >> 2) & 63, t = (e >> 8) % kNwTiles, w = (e >> 8) / kNwTiles;
  const int o = 32 * (w >> 2) + 16 * (t / 9) + 4 * (l >> 4) + i, c = 16 * (w & 3) + (l & 15), tap = t % 9;
  float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  int g = 0;
  for (; g + 8 <= G; g += 8) {
#pragma unroll
    for (int j = 0; j < 8; ++j) s[j] += part[(size_t)(g + j) * kNwPer + e];
  }
  for (int j = 0; g < G; ++g, ++j) s[j] += part[(size_t)g * kNwPer + e];
  dw[(o * 64 + c) * 9 + tap] = ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]));
}

inline bool np_a16(const void* p) { return ((uintptr_t)p & 15u) == 0; }
inline int nw_grid(int B, int T) {  // workgroups of the weight gradient: one per trip, at most one per CU
  const int trips = (B + T - 1) / T;
  return trips < kNwGrid ? (trips > 0 ? trips : 1) : kNwGrid;
}

template <int N>
int conv_np_launch(const float* x, int B, const void* wsplit, const float* inv, const float* bias, float* y,
                   hipStream_t s) {
  using G = NcGeo<N>;
  const void* fns[1] = {(const void*)k_conv_x3_np<N>};
  if (set_max_dynamic_lds(fns, 1, G::LDS) != BK_OK) return BK_EHIP;
  const int ntiles = (B + G::T - 1) / G::T;
  const int grid = ntiles < 256 ? ntiles : 256;  // persistent: one workgroup per CU, tiles strided
  hipLaunchKernelGGL(k_conv_x3_np<N>, dim3(grid), dim3(kLnThreads), G::LDS, s, x, (const h16x8*)wsplit, inv, bias, y, B);
  return launch_check("k_conv_x3_np");
}

template <int N>
int wgrad_np_launch(const float* x, const float* dy, int B, float* workspace, float* dw, hipStream_t s) {
  using G = NwGeo<N>;
  const void* fns[1] = {(const void*)k_conv_x3_np_wgrad<N>};
  if (set_max_dynamic_lds(fns, 1, G::LDS) != BK_OK) return BK_EHIP;
  const int grid = nw_grid(B, G::T);
  hipLaunchKernelGGL(k_conv_x3_np_wgrad<N>, dim3(grid), dim3(kNwThreads), G::LDS, s, x, dy, B, (f32x4*)workspace);
  if (launch_check("k_conv_x3_np_wgrad") != BK_OK) return BK_EHIP;
  hipLaunchKernelGGL(k_conv_x3_np_wgrad_reduce, dim3((kNwPer + 255) / 256), dim3(256), 0, s, workspace, grid, dw);
  return launch_check("k_conv_x3_np_wgrad_reduce");
}

}  // namespace
}  // namespace bk

using namespace bk;

extern "C" {

int bk_conv_x3_np_supported(int N) { return N == 7 || N == 14 ? 1 : 0; }

int bk_conv_x3_np_tile_boards(int N) { return N == 7 ? NcGeo<7>::T : N == 14 ? NcGeo<14>::T : 0; }

int bk_conv_x3_np(const float* x, int B, int N, const void* wsplit, const float* inv, const float* bias, float* y,
                  void* stream) {
  BK_REQUIRE(x && wsplit && inv && y && B >= 0, "bad argument");
  BK_REQUIRE(N == 7 || N == 14, "bk_conv_x3_np: 7x7 or 14x14 boards");
  BK_REQUIRE(np_a16(x) && np_a16(wsplit) && np_a16(inv) && np_a16(y) && (!bias || np_a16(bias)),
             "bk_conv_x3_np: 16-byte aligned buffers");
  BK_REQUIRE((long long)B * N * N * 16 < (1ll << 31), "bk_conv_x3_np: batch too large");
  if (B == 0) return BK_OK;
  hipStream_t s = (hipStream_t)stream;
  return N == 7 ? conv_np_launch<7>(x, B, wsplit, inv, bias, y, s) : conv_np_launch<14>(x, B, wsplit, inv, bias, y, s);
}

int bk_conv_x3_np_wgrad_tile_boards(int N) { return N == 7 ? NwGeo<7>::T : N == 14 ? NwGeo<14>::T : 0; }

int bk_conv_x3_np_wgrad_workspace_floats(int B, int N) {
  if (N != 7 && N != 14) return 0;
  return nw_grid(B, N == 7 ? NwGeo<7>::T : NwGeo<14>::T) * kNwPer;
}

int bk_conv_x3_np_wgrad(const float* x, const float* dy, int B, int N, float* workspace, float* dw, void* stream) {
  BK_REQUIRE(dw && B >= 0 && (B == 0 || (x && dy && workspace)), "bad argument");
  BK_REQUIRE(N == 7 || N == 14, "bk_conv_x3_np_wgrad: 7x7 or 14x14 boards");
  BK_REQUIRE(np_a16(x) && np_a16(dy) && np_a16(workspace), "bk_conv_x3_np_wgrad: 16-byte aligned buffers");
  BK_REQUIRE((long long)B * N * N * 16 < (1ll << 31), "bk_conv_x3_np_wgrad: batch too large");
  hipStream_t s = (hipStream_t)stream;
  if (B == 0) return hipMemsetAsync(dw, 0, 64 * 64 * 9 * sizeof(float), s) == hipSuccess ? BK_OK : BK_EHIP;
  return N == 7 ? wgrad_np_launch<7>(x, dy, B, workspace, dw, s) : wgrad_np_launch<14>(x, dy, B, workspace, dw, s);
}

}  // extern "C"

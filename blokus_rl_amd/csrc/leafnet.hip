// leafnet.hip — the leaf ResNet (models/blokus_nnet.py:88-151, eval-mode BN folded) of one board
// per workgroup, on the f16 matrix cores with fp32-class accuracy ("x3" = three f16 products).
//
// Why: the f32 MFMA (v_mfma_f32_16x16x4_f32) runs at 1/16 of the f16 rate on gfx950 and does not
// overlap the VALU, so the round-1 tower (Winograd on f32 MFMA, conv.hip) was bound at ~57% of a
// low peak. Here every operand x (weights and activations, fp32) is split into two f16 halves
// x = hi + lo (hi = f16(x), lo = f16(x - hi): 22 significant bits) and each product is taken as
// hi*hi + lo*hi + hi*lo on v_mfma_f32_16x16x32_f16 (exact f16 products, f32 accumulation); the
// dropped lo*lo term is below 2^-22 of the product. To keep both halves normal f16 numbers, the
// operands are scaled by powers of two first: the weights per output channel on the host (largest
// |w| in [2^14, 2^15)), the activations per board and layer on the device (the largest |x| of the
// board's layer input in [2^14, 2^15)); the accumulator is unscaled exactly by the inverse powers.
// Measured error against an fp64 forward: tests/test_leafnet_gpu.py (same order as the fp32 kernel).
//
// Convolutions are direct (implicit GEMM): M = 16 output channels per wave (4 waves = 64), N = 16
// pixels per group (NG = ceil(N*N/16) groups cover the board), K = 9 taps x Cin in chunks of 32
// (tap t = c/2, channel half c%2 for Cin = 64; taps 4c..4c+3 x 8 channels for the stem). The
// board's layer input lives in LDS as zero-haloed pixel grids of split halves, one plane per
// 8 channels (ln_plane): the B fragment of lane l is one ds_read_b128 per half at the slot of
// column l%16 of group g (LnPixMap) shifted by the tap, in the plane of channels 8(l/16).. of
// the chunk. The A fragments
// (weights) stream from global memory (L2-resident across the 32 boards of an XCD), one chunk
// ahead. The accumulators of all NG groups stay in registers for the layer; the epilogue applies
// scale, bias, (residual), ReLU, finds the board maximum, splits and writes the next layer input
// in place. The stem output x0 stays in registers for the tower's final residual, and the last
// layer's epilogue feeds the heads' 1x1 convs straight from the registers.
#include "../../include/blokus_engine.h"
#include "ctx.h"

#include <string>
#include <type_traits>

// the MFMA accumulators in VGPRs: the epilogue's VALU reads them without 100 v_accvgpr_read per
// layer (AGPRs: 159.7 vs 157.9 us a launch, self-play +0.9%, three interleaved rounds on one box;
// x0 still waits in AGPRs)
#define BK_LN_VACC 1
#include "leafnet_common.h"

namespace bk {
namespace {

// The kernel's input form: the planar observation [B][8][N][N] f32 (as k_observe / the search
// write it), or (STATES) the packed states it is made from, [B][kStateWords] words, with the
// search's leaf status per board (null: every board is a leaf).
struct LnStates {
  const uint32_t* states;
  const int32_t* status;
};
constexpr int kLnP = kStemCinX3 / 2;        // players of the 8-plane observation
constexpr int kLnRowWords = kLnP * kMaxN;   // a state's board rows: plane p, row r = word p * kMaxN + r

// FAST heads: the 1x1 convs' lane sums for the two policy channels at once, as packed f32 ops:
// {y . w0, y . w1} with wx = {w0.x, w1.x} ... ww = {w0.w, w1.w}; each half is the plain
// ((y.x w.x + y.y w.y) + y.z w.z) + y.w w.w (separate multiplies and adds, in that order).
__device__ __forceinline__ f32x2 ln_dot2(f32x4 y, f32x2 wx, f32x2 wy, f32x2 wz, f32x2 ww) {
  const f32x2 xy{y.x, y.y}, zw{y.z, y.w};
  f32x2 t, u;
  asm("v_pk_mul_f32 %0, %1, %2 op_sel:[0,0] op_sel_hi:[0,1]" : "=v"(t) : "v"(xy), "v"(wx));
  asm("v_pk_mul_f32 %0, %1, %2 op_sel:[1,0] op_sel_hi:[1,1]" : "=v"(u) : "v"(xy), "v"(wy));
  t = pk_add(t, u);
  asm("v_pk_mul_f32 %0, %1, %2 op_sel:[0,0] op_sel_hi:[0,1]" : "=v"(u) : "v"(zw), "v"(wz));
  t = pk_add(t, u);
  asm("v_pk_mul_f32 %0, %1, %2 op_sel:[1,0] op_sel_hi:[1,1]" : "=v"(u) : "v"(zw), "v"(ww));
  return pk_add(t, u);
}
// FAST heads: the sums over the wave's 4 k-groups (rows of 16 lanes) of four values at once. Row
// r of the result holds v_r summed as (row 0 + row 1) + (row 2 + row 3), the order of the
// one-value form a + a(lane ^ 16), then + (lane ^ 32) (x + y is the same sum in either order):
// v_permlane16_swap pairs v0 with v1 and v2 with v3 (even rows keep the first value's rows 0 / 2
// and take its rows 1 / 3 as the addend, odd rows the second value's), v_permlane32_swap then
// pairs the two results' halves: 3 swaps and 3 adds for four values instead of 8 and 8.
__device__ __forceinline__ float ln_quad_sum(float v0, float v1, float v2, float v3) {
  const auto s01 = __builtin_amdgcn_permlane16_swap(__float_as_uint(v0), __float_as_uint(v1), false, false);
  const float a = __uint_as_float(s01[0]) + __uint_as_float(s01[1]);
  const auto s23 = __builtin_amdgcn_permlane16_swap(__float_as_uint(v2), __float_as_uint(v3), false, false);
  const float c = __uint_as_float(s23[0]) + __uint_as_float(s23[1]);
  const auto s = __builtin_amdgcn_permlane32_swap(__float_as_uint(a), __float_as_uint(c), false, false);
  return __uint_as_float(s[0]) + __uint_as_float(s[1]);
}

// FAST stem on a board without a lo plane: ln_chunk_hi with each group's B-fragment read (kLnPf
// groups ahead) issued between its two MFMAs in one asm block, as ln_chunk_il does for the tower:
// wait (lgkmcnt(kLnPf - 1): only the reads of the blocks between may still be in flight), MFMA,
// read, MFMA. The stem's tap offset differs per lane (tap 4j + ks), so the read takes its whole
// address from a register. Same discipline as ln_chunk_il: the ring registers are only read by
// later blocks, after their wait, and the caller waits lgkmcnt(0) after the last chunk. Same
// MFMAs on the same operands as ln_chunk_hi: the sums are bitwise equal.
template <int NG, bool INIT>
__device__ __forceinline__ void ln_chunk_hi_il(f32x4 (&acc)[NG], h16x8 ah, h16x8 al, const unsigned char* grid,
                                               const int (&pb)[NG], int coff, int coff_next, h16x8 (&rb)[kLnSlots][2]) {
  static_assert(NG % kLnSlots == 0, "ln_chunk_hi_il: the ring slot of a group must not depend on the chunk");
  const unsigned gbase = (unsigned)(uintptr_t)grid;
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    const int gp = g + kLnPf;
    const unsigned addr = gbase + (unsigned)(gp < NG ? pb[gp] + coff : pb[gp - NG] + coff_next);
    h16x8& n0 = rb[gp % kLnSlots][0];
    if (INIT)
      asm volatile(
          "s_waitcnt lgkmcnt(%6)\n\t"
          "v_mfma_f32_16x16x32_f16 %0, %2, %4, 0\n\t"
          "ds_read_b128 %1, %5\n\t"
          "v_mfma_f32_16x16x32_f16 %0, %3, %4, %0"
          : BK_ACC_W(acc[g]), "=&v"(n0)
          : "v"(ah), "v"(al), "v"(rb[g % kLnSlots][0]), "v"(addr), "i"(kLnPf - 1));
    else
      asm volatile(
          "s_waitcnt lgkmcnt(%6)\n\t"
          "v_mfma_f32_16x16x32_f16 %0, %2, %4, %0\n\t"
          "ds_read_b128 %1, %5\n\t"
          "v_mfma_f32_16x16x32_f16 %0, %3, %4, %0"
          : BK_ACC_RW(acc[g]), "=&v"(n0)
          : "v"(ah), "v"(al), "v"(rb[g % kLnSlots][0]), "v"(addr), "i"(kLnPf - 1));
  }
}

// Test hook of the FAST planes form (bk_ln_path_counts): while [0] is set, each workgroup counts the
// stem it takes, [1] the two-product stem of a binary board, [2] the full stem. The flag is one
// scalar load in flight under the observation loads.
__device__ unsigned g_ln_paths[3];

// STATES: the stem input is built from the board's state words instead of read as floats. Every
// plane of the observation is binary (k_observe, env.hip), so the scaled board is 2^ex where a bit
// is set and 0 elsewhere, ex = scale_exp(1) (scale_exp(0) on an all-zero board), and its lo half
// is identically zero: only the hi plane is built and the stem takes two products per chunk
// (ln_chunk_hi). The accumulators, and so every output, equal the planar form's on
// bk_observe(states) as float values. A board whose status is not 1 (no leaf for the net: its
// state row is stale) is the all-zero observation, as the search writes it in the planar form;
// its state words are not loaded.
//
// EDGE (N = 20, the default: BK_LN_EDGE): the pixels sit in MFMA columns by LnEdgePixMap, whose
// last four groups are pieces of the four board edges, and the tower's chunk loop follows
// LnEdgeSched: each of those groups leaves out the 6 of 18 chunks whose tap reads only the zero
// halo (24 of a conv's 450 (group, chunk) pairs, 72 of 1350 MFMAs per wave with their 48
// ds_read_b128). The products left out are a*0: every output is bitwise the full schedule's
// (leafnet_common.h ln_chunk_il_act). The stem (4 taps per chunk: nothing to skip) only takes the map.
//
// FAST (the default: BK_LN_FAST): the shorter stem, prologue and heads below, every output bitwise
// what the other instantiation computes. Planes form: a board whose 16 floats per lane are all
// exactly 0.0f or 1.0f (every observation the search writes) has an all-zero lo plane, so it takes
// the STATES form's two-product stem on the hi plane alone; any other board takes the full stem
// (a workgroup-uniform branch). The halo is zeroed from per-thread constant slots, the STATES form
// loads its state words without waiting for status[b], the stem's epilogue makes x0 and the split
// halves in one pass and stores them as made (one barrier instead of two), and the heads reduce
// four pixel groups' 1x1 sums at a time into a scratch indexed by grid slot, issue every later
// global load before their first barrier and take one tanh for all value outputs.
template <int N, typename In, bool EDGE_A = false, bool FAST = false>  // In: const float* (planes), LnStates or LnRows
__global__ __launch_bounds__(kLnThreads, 1) void k_leafnet_x3(In in,
                                                              const h16x8* __restrict__ wstem_a,
                                                              const float* __restrict__ sstem_a,
                                                              const float* __restrict__ bstem_a,
                                                              const h16x8* __restrict__ wt_a,
                                                              const float* __restrict__ st_a,
                                                              const float* __restrict__ bt_a,
                                                              const float* __restrict__ bounds_a, int nlayers,
                                                              LnHeads hd_a, float* __restrict__ xout) {
  // ROWS (bk_leafnet_x3_rows): the STATES form on state row tree[blockIdx.x] with the row's own
  // weight set; the *_a weight arguments are unused (null) and the operands below come from the
  // table in `in`. The other forms take the arguments as they are.
  constexpr bool ROWS = std::is_same<In, LnRows>::value;
  constexpr bool STATES = std::is_same<In, LnStates>::value || ROWS;
  constexpr bool EDGE = EDGE_A;
  const h16x8* __restrict__ wstem = wstem_a;
  const float* __restrict__ sstem = sstem_a;
  const float* __restrict__ bstem = bstem_a;
  const h16x8* __restrict__ wt = wt_a;
  const float* __restrict__ st = st_a;
  const float* __restrict__ bt = bt_a;
  const float* __restrict__ bounds = bounds_a;
  LnHeads hd = hd_a;
  size_t b = blockIdx.x;
  if constexpr (ROWS) {
    // workgroup-uniform, before any barrier or LDS use
    int k;
    const int t = ln_row_tree(in, blockIdx.x, k);
    if (t < 0) return;
    b = (size_t)t;
    const LnNet nk = ln_pick(in.nets, k);
    wstem = nk.wstem;
    sstem = nk.sstem;
    bstem = nk.bstem;
    wt = nk.wt;
    st = nk.st;
    bt = nk.bt;
    bounds = nk.bounds;
    hd.wp = nk.wp;
    hd.bp = nk.bp;
    hd.wv = nk.wv;
    hd.bv = nk.bv;
    hd.w1t = nk.w1t;
    hd.b1 = nk.b1;
    hd.w2 = nk.w2;
    hd.b2 = nk.b2;
  }
  constexpr int NN = N * N, RS = ln_row(N), NG = ln_groups(N), PIX_IT = (NN + kLnThreads - 1) / kLnThreads;
  constexpr int PL = ln_plane(N);
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  unsigned char* act = lds;                  // 16 planes [hi q | lo q][(N+2) x RS slots][16 B]
  unsigned char* sin = lds + 16 * PL;        // 2 planes: the stem input hi, lo
  float* red = reinterpret_cast<float*>(lds + ln_lds_body(N));
  constexpr int X0L = ln_x0_lds_groups(N);   // x0 groups 0..X0L-1 stashed in LDS
  f32x4* x0s = reinterpret_cast<f32x4*>(lds + 16 * PL);
  const int tid = threadIdx.x, l = tid & 63, n = l & 15, ks = l >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform
  const int oc = 16 * wave + 4 * ks;  // the lane's 4 output channels oc..oc+3 in the D fragments
  LNSTAMP(0, __builtin_amdgcn_s_memtime());
  LNSTAMP(30, __builtin_amdgcn_s_memrealtime());

  // the observation loads first (their latency under the halo zeroing below)
  float xin[STATES ? 1 : PIX_IT][kStemCinX3];
  uint32_t sw = 0u;  // STATES: thread tid < kLnRowWords holds row word tid, thread kLnRowWords to_move
  bool live = true;
  bool count_paths = false;
  if constexpr (STATES) {
    static_assert(kLnRowWords < kLnThreads && N <= kMaxN, "k_leafnet_x3: one state word per thread");
    if constexpr (FAST && !ROWS) {
      // the state words do not wait for status[b]: both loads are in flight together, and the words
      // of a board that is not a leaf (stale, but valid memory) are dropped
      if (tid <= kLnRowWords) sw = in.states[b * kStateWords + (tid < kLnRowWords ? tid : kWToMove)];
      live = !in.status || in.status[b] == 1;
      if (!live) sw = 0u;
    } else {
      live = ROWS || !in.status || in.status[b] == 1;  // ROWS: a leaf, or the workgroup has returned
      if (live && tid <= kLnRowWords) sw = in.states[b * kStateWords + (tid < kLnRowWords ? tid : kWToMove)];
    }
  } else {
    if constexpr (FAST) count_paths = g_ln_paths[0] != 0u;
    const float* __restrict__ ob = in + b * kStemCinX3 * NN;
#pragma unroll
    for (int it = 0; it < PIX_IT; ++it) {
      const int p = tid + it * kLnThreads;
#pragma unroll
      for (int c = 0; c < kStemCinX3; ++c) xin[it][c] = p < NN ? ob[c * NN + p] : 0.0f;
    }
  }
  // zero the halo of all 18 planes (rows 0 and N+1, columns 0 and N+1..RS-1; the only slots read
  // that no layer writes: interiors are written before they are read); STATES: 17, the stem
  // input has no lo plane
  constexpr int kHaloCols = RS - N, kHalo = 2 * RS + N * kHaloCols;
  // FAST: thread tid owns halo slot tid % kHalo in the planes of its set tid / kHalo (plane = set,
  // set + kHaloSets, ...): one decode per thread, then a store per plane at a constant stride. The
  // planes form leaves out the stem's lo plane here: a binary board never reads it, any other
  // board zeroes its halo beside the interior writes.
  constexpr int kHaloSets = kLnThreads / kHalo;
  static_assert(kHaloSets >= 1, "k_leafnet_x3: a plane's halo slots fit the workgroup");
  int halo_off = -1;  // the thread's halo slot in a plane, bytes (-1: none)
  if constexpr (FAST) {
    const int set = tid / kHalo, k = tid - set * kHalo;
    int row, col;
    if (k < 2 * RS) {
      row = k < RS ? 0 : N + 1;
      col = k < RS ? k : k - RS;
    } else {
      const int h = k - 2 * RS, c = h % kHaloCols;
      row = 1 + h / kHaloCols;
      col = c == 0 ? 0 : N + c;
    }
    if (set < kHaloSets) {
      halo_off = (row * RS + col) * 16;
      unsigned char* q = lds + set * PL + halo_off;
#pragma unroll
      for (int j = 0; j * kHaloSets < 17; ++j)
        if (j * kHaloSets + set < 17) *reinterpret_cast<u32x4*>(q + j * kHaloSets * PL) = u32x4{0u, 0u, 0u, 0u};
    }
  } else {
    for (int i = tid; i < (STATES ? 17 : 18) * kHalo; i += kLnThreads) {
      const int plane = i / kHalo, k = i - plane * kHalo;
      int row, col;
      if (k < 2 * RS) {
        row = k < RS ? 0 : N + 1;
        col = k < RS ? k : k - RS;
      } else {
        const int h = k - 2 * RS, c = h % kHaloCols;
        row = 1 + h / kHaloCols;
        col = c == 0 ? 0 : N + c;
      }
      *reinterpret_cast<u32x4*>(lds + plane * PL + (row * RS + col) * 16) = u32x4{0u, 0u, 0u, 0u};
    }
  }
  LNSTAMP(32, __builtin_amdgcn_s_memtime());

  // the lane's grid slot in each group, in bytes (a spare column reads slot 0 of the halo: zeros),
  // and the mask of groups where the lane's column is a board pixel
  // ab[g] = the lane's B-read base: its slot + its k-group's plane block, less kBias so that
  // every chunk's plane/tap offset is a non-negative immediate (no address VALU in the MFMA loop);
  // a spare column reads at pixel (0, 0) (its MFMA column is never written out)
  constexpr int kBias = (RS + 1) * 16;
  int ab[NG];
  unsigned valid = 0;
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    int sl;
    if constexpr (EDGE)
      sl = kLnEdgePixMap<N>.slot[16 * g + n];
    else
      sl = kLnPixMap<N>.slot[16 * g + n];
    ab[g] = (sl >= 0 ? sl : RS + 1) * 16 + ks * 4 * PL - kBias;
    valid |= (sl >= 0 ? 1u : 0u) << g;
  }
  auto is_valid = [&](int g) { return NN % 16 == 0 || ((valid >> g) & 1u); };
  auto slot_b = [&](int g) { return ab[g] - ks * 4 * PL + kBias; };  // the lane's slot in group g, bytes

  // the weights stream through a ring of kLnWpf + 1 chunks, kLnWpf chunks ahead of the MFMAs and
  // on into the next layer (18 chunks per layer: the ring slot of chunk c is c % (kLnWpf + 1) in
  // every layer), so no layer starts on an exposed L2 load
  static_assert(18 % (kLnWpf + 1) == 0, "kLnWpf: the ring must divide the 18 chunks of a layer");
  constexpr int kLayerBlocks = 18 * 4 * 2;  // (chunk, wave, part) blocks of 64 x 16 B per layer
  const __amdgpu_buffer_rsrc_t wrs = ln_rsrc(wt, (unsigned)nlayers * kLayerBlocks * 1024u);
  // part p (0 hi, 1 lo) of the lane's A fragment of chunk c of tower layer `layer`
  auto wload = [&](int layer, int c, int p) {
    return __builtin_bit_cast(h16x8, __builtin_amdgcn_raw_buffer_load_b128(
                                         wrs, l * 16, ((layer * kLayerBlocks + c * 8 + wave * 2 + p) * 64) * 16, 0));
  };
  h16x8 wq[kLnWpf + 1][2];  // issued here: in flight under the stem
#pragma unroll
  for (int c = 0; c < kLnWpf; ++c) {
    wq[c][0] = wload(0, c, 0);
    wq[c][1] = wload(0, c, 1);
  }
  // the stem's weights (3 chunks), scale and bias, in flight under the observation loads
  h16x8 wsa[3][2];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    wsa[j][0] = wstem[((j * 4 + wave) * 2) * 64 + l];
    wsa[j][1] = wstem[((j * 4 + wave) * 2 + 1) * 64 + l];
  }
  const f32x4 s_stem = *reinterpret_cast<const f32x4*>(sstem + oc), b_stem = *reinterpret_cast<const f32x4*>(bstem + oc);

  // ---- stem input: the planar observation [8][N][N] of the board, scaled by its maximum, split
  float max_obs;
  int ex;
  bool binary = STATES;  // the stem input has no lo plane (workgroup-uniform)
  if constexpr (STATES) {
    // the board's row words (bits past the board dropped, as the observation drops them) and
    // to_move staged in the unused lo plane's space; the board maximum is 1 iff any plane has a
    // cell set: a row bit, or a to_move that names one of the kLnP mover planes
    uint32_t* rows = reinterpret_cast<uint32_t*>(sin + PL);
    bool any = false;
    if (tid < kLnRowWords) {
      const uint32_t bits = tid % kMaxN < N ? sw & ((1u << N) - 1u) : 0u;
      rows[tid] = bits;
      any = bits != 0u;
    } else if (tid == kLnRowWords) {
      const uint32_t tm = live ? sw : ~0u;  // no mover plane of a board that is not a leaf
      rows[kLnRowWords] = tm;
      any = tm < (uint32_t)kLnP;
    }
    max_obs = block_max(any ? 1.0f : 0.0f, red + 8, wave, l);  // the barrier: zeroing and rows before the writes
    ex = scale_exp(max_obs);
    LNSTAMP(36, __builtin_amdgcn_s_memtime());
    // a set cell's hi half: f16(2^ex), what split2 gives the planar form's 1.0f * 2^ex
    const unsigned one = __builtin_bit_cast(unsigned short, (_Float16)ldexpf(1.0f, ex));
    const uint32_t tm = rows[kLnRowWords];
    const unsigned m01 = ((tm == 0u ? 1u : 0u) | (tm == 1u ? 0x10000u : 0u)) * one;
    const unsigned m23 = ((tm == 2u ? 1u : 0u) | (tm == 3u ? 0x10000u : 0u)) * one;
#pragma unroll
    for (int it = 0; it < PIX_IT; ++it) {
      const int p = tid + it * kLnThreads;
      if (p < NN) {
        const int r = p / N, c = p % N;
        unsigned bit[kLnP];
#pragma unroll
        for (int q = 0; q < kLnP; ++q) bit[q] = (rows[q * kMaxN + r] >> c) & 1u;
        // channels 2q (low 16 bits), 2q + 1 (high) per word, as split2 packs them
        const u32x4 hi{(bit[0] | (bit[1] << 16)) * one, (bit[2] | (bit[3] << 16)) * one, m01, m23};
        *reinterpret_cast<u32x4*>(sin + ((r + 1) * RS + c + 1) * 16) = hi;
      }
    }
  } else {
    float m = 0.0f;
#pragma unroll
    for (int it = 0; it < PIX_IT; ++it)
#pragma unroll
      for (int c = 0; c < kStemCinX3; ++c) m = fmaxf(m, fabsf(xin[it][c]));
    if constexpr (FAST) {
      // the lane's floats are all exactly 0.0f or 1.0f (-0.0f and every other value fail); the
      // workgroup's AND rides in the maximum's reduction (its own 4 floats of red, no barrier more)
      bool bin = true;
#pragma unroll
      for (int it = 0; it < PIX_IT; ++it)
#pragma unroll
        for (int c = 0; c < kStemCinX3; ++c) {
          const unsigned u = __float_as_uint(xin[it][c]);
          bin = bin && (u == 0u || u == 0x3F800000u);
        }
      const bool wbin = __builtin_amdgcn_ballot_w64(!bin) == 0ull;
      if (l == 0) red[12 + wave] = wbin ? 1.0f : 0.0f;
    }
    max_obs = block_max(m, red + 8, wave, l);  // the barrier also orders the zeroing before the writes
    ex = scale_exp(max_obs);
    LNSTAMP(36, __builtin_amdgcn_s_memtime());
    if constexpr (FAST) {
      const uint4 f = *reinterpret_cast<const uint4*>(red + 12);
      binary = __builtin_amdgcn_readfirstlane((f.x & f.y & f.z & f.w) != 0u) != 0;
      if (count_paths && tid == 0) atomicAdd(&g_ln_paths[binary ? 1 : 2], 1u);
    }
    if (FAST && binary) {
      // x 2^ex is 0 or 2^ex, an f16 number: the hi half is the value, the lo half +0 in every cell
      const _Float16 one = (_Float16)ldexpf(1.0f, ex);
#pragma unroll
      for (int it = 0; it < PIX_IT; ++it) {
        const int p = tid + it * kLnThreads;
        if (p < NN) {
          unsigned h[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const h16x2 v = h16x2{(_Float16)xin[it][2 * q], (_Float16)xin[it][2 * q + 1]} * h16x2{one, one};
            h[q] = __builtin_bit_cast(unsigned, v);
          }
          *reinterpret_cast<u32x4*>(sin + ((p / N + 1) * RS + p % N + 1) * 16) = u32x4{h[0], h[1], h[2], h[3]};
        }
      }
    } else {
      if (FAST && tid < kHalo) *reinterpret_cast<u32x4*>(sin + PL + halo_off) = u32x4{0u, 0u, 0u, 0u};  // the lo plane's halo
#pragma unroll
      for (int it = 0; it < PIX_IT; ++it) {
        const int p = tid + it * kLnThreads;
        if (p < NN) {
          unsigned h[4], o[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) split2(ldexpf(xin[it][2 * q], ex), ldexpf(xin[it][2 * q + 1], ex), h[q], o[q]);
          const u32x4 hi{h[0], h[1], h[2], h[3]}, lo{o[0], o[1], o[2], o[3]};
          unsigned char* dst = sin + ((p / N + 1) * RS + p % N + 1) * 16;
          *reinterpret_cast<u32x4*>(dst) = hi;
          *reinterpret_cast<u32x4*>(dst + PL) = lo;
        }
      }
    }
  }
  LNSTAMP(33, __builtin_amdgcn_s_memtime());
  __syncthreads();
  LNSTAMP(1, __builtin_amdgcn_s_memtime());

  // ---- stem conv: 3 chunks; lane k-group ks of chunk j is tap 4j + ks (taps > 8 carry zero weights)
  f32x4 acc[NG];
  h16x8 rb[kLnSlots][2];
  {
    auto toff = [&](int j) {
      const int t = 4 * j + ks < 9 ? 4 * j + ks : 8;
      return ((t / 3 - 1) * RS + (t % 3 - 1)) * 16 + kBias - ks * 4 * PL;  // from ab: the stem grid has 2 planes
    };
    if (binary) {  // no lo plane: two products per chunk
      ln_prime_hi<NG>(rb, sin, ab, toff(0));
      if constexpr (FAST) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the primed reads: the blocks below count their own
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          if (j == 0)
            ln_chunk_hi_il<NG, true>(acc, wsa[0][0], wsa[0][1], sin, ab, toff(0), toff(1), rb);
          else
            ln_chunk_hi_il<NG, false>(acc, wsa[j][0], wsa[j][1], sin, ab, toff(j), toff(j < 2 ? j + 1 : j), rb);
        }
        // the last chunk's read-ahead (untracked) lands before its registers are reused
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      } else {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          if (j == 0)
            ln_chunk_hi<NG, true>(acc, wsa[0][0], wsa[0][1], sin, ab, toff(0), toff(1), rb);
          else
            ln_chunk_hi<NG, false>(acc, wsa[j][0], wsa[j][1], sin, ab, toff(j), toff(j < 2 ? j + 1 : j), rb);
        }
      }
    } else {
      ln_prime<NG, PL>(rb, sin, ab, toff(0));
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        if (j == 0)
          ln_chunk<NG, true, PL>(acc, wsa[0][0], wsa[0][1], sin, ab, toff(0), toff(1), rb);
        else
          ln_chunk<NG, false, PL>(acc, wsa[j][0], wsa[j][1], sin, ab, toff(j), toff(j < 2 ? j + 1 : j), rb);
      }
    }
  }
  ln_mfma_drain(acc);
  LNSTAMP(2, __builtin_amdgcn_s_memtime());

  // Epilogue of a conv: y = acc * s + bias (+ x0) (ReLU), s = the inverse weight scale x 2^-ex_in.
  // OUT: y is the next layer's input: scaled by 2^ex_out (ex_out from a bound on |y|, so no board
  // reduction is needed before the split), split, and the packed halves kept in acc's registers
  // until every wave has finished reading the grid (bar 1), then written; the lane's max |y|
  // (unscaled) is returned for the next layer's bound. !OUT (the last conv): y stays in acc.
  // WRITE (with OUT, after a barrier that every wave has finished reading the grid): each group's
  // halves are stored into the grid as soon as they are split, so the LDS stores drain under the
  // next groups' VALU instead of after all of it.
  auto epilogue = [&](f32x4 sv, f32x4 bv, bool relu, bool residual, const f32x4 (&x0)[NG], bool out, int ex_out,
                      bool write = false) {
    const int o = 2 * wave + (ks >> 1);
    unsigned char* wbase = act + ((o & 3) * 4 + (o >> 2) * 2) * PL + (ks & 1) * 8;  // as write_act
    // OUT folds the output scale 2^ex_out into s and bias (exact: powers of two), so y comes out
    // scaled and goes straight to the split; the lane maximum is unscaled once at the end
    const int k = out ? ex_out : 0;
    const f32x2 s01{ldexpf(sv.x, k - ex), ldexpf(sv.y, k - ex)}, s23{ldexpf(sv.z, k - ex), ldexpf(sv.w, k - ex)};
    const f32x2 b01{ldexpf(bv.x, k), ldexpf(bv.y, k)}, b23{ldexpf(bv.z, k), ldexpf(bv.w, k)};
    const int floor = relu ? 0 : (int)0x80000000u;
    float mx = 0.0f;
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      f32x2 y01 = pk_fma(f32x2{acc[g][0], acc[g][1]}, s01, b01);
      f32x2 y23 = pk_fma(f32x2{acc[g][2], acc[g][3]}, s23, b23);
      if (residual) {  // only without OUT (the last conv): x0 is unscaled
        y01 = pk_add(y01, f32x2{x0[g][0], x0[g][1]});
        y23 = pk_add(y23, f32x2{x0[g][2], x0[g][3]});
      }
      y01 = f32x2{max_bits(y01.x, floor), max_bits(y01.y, floor)};
      y23 = f32x2{max_bits(y23.x, floor), max_bits(y23.y, floor)};
      if (is_valid(g)) mx = max3_abs(max3_abs(mx, y01.x, y01.y), y23.x, y23.y);
      if (out) {
        unsigned h0, h1, l0, l1;
        split2(y01.x, y01.y, h0, l0);
        split2(y23.x, y23.y, h1, l1);
        if (write) {
          if (is_valid(g)) {
            *reinterpret_cast<u32x2*>(wbase + slot_b(g)) = u32x2{h0, h1};
            *reinterpret_cast<u32x2*>(wbase + slot_b(g) + PL) = u32x2{l0, l1};
          }
        } else {
          acc[g] = f32x4{__builtin_bit_cast(float, h0), __builtin_bit_cast(float, h1), __builtin_bit_cast(float, l0),
                         __builtin_bit_cast(float, l1)};
        }
      } else {
        acc[g] = f32x4{y01.x, y01.y, y23.x, y23.y};
      }
    }
    return ldexpf(mx, -k);
  };
  // the packed halves in acc -> the activation grid. The lane holds channels oc..oc+3 (hi, lo) of
  // octet o = 2 wave + ks/2; the k-groups ks and ks^1 (rows of 16 lanes) hold the two halves of the
  // octet's 16-B slot. v_permlane16_swap gives the even row both rows' hi halves and the odd row
  // both lo halves, so each lane stores one 16-B slot (hi plane, or the lo plane next to it).
  auto write_act = [&]() {
    const int o = 2 * wave + (ks >> 1);
    // each lane stores its 4 channels' hi and lo halves (8 B each) into its half of the octet's
    // 16-B slot in the hi plane and in the lo plane (no lane swaps)
    unsigned char* base = act + ((o & 3) * 4 + (o >> 2) * 2) * PL + (ks & 1) * 8;
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      const u32x4 w = __builtin_bit_cast(u32x4, acc[g]);  // {hi 01, hi 23, lo 01, lo 23}
      if (is_valid(g)) {
        *reinterpret_cast<u32x2*>(base + slot_b(g)) = u32x2{w.x, w.y};
        *reinterpret_cast<u32x2*>(base + slot_b(g) + PL) = u32x2{w.z, w.w};
      }
    }
  };
  // the scale of a conv's output from the bound |y| <= A max_in + B (A = the largest row L1 norm
  // of the weights, B = the largest |bias|: nets.pack_x3)
  auto out_exp = [&](int conv, float max_in) { return scale_exp(bounds[2 * conv] * max_in + bounds[2 * conv + 1]); };
  // wave maxima -> red[par][wave] before the barrier, the board maximum after it
  auto post_max = [&](float mx, int par) {
    mx = wave_max_f(mx);
    if (l == 0) red[4 * par + wave] = mx;
  };
  auto board_max = [&](int par) {
    return fmaxf(fmaxf(red[4 * par], red[4 * par + 1]), fmaxf(red[4 * par + 2], red[4 * par + 3]));
  };

  f32x4 x0[NG];
  float max_in;
  if constexpr (FAST) {
    // one pass: y (= x0[g], unscaled), y 2^ex_out (exact), its split halves, stored into the grid
    // as they are made: no wave reads the activation planes before the barrier below (the stem
    // reads its own two), so only the x0 stash, which reuses those two, waits for it; the stash is
    // read back by its own thread alone
    const int ex_out = out_exp(0, max_obs);
    const int o = 2 * wave + (ks >> 1);
    unsigned char* wbase = act + ((o & 3) * 4 + (o >> 2) * 2) * PL + (ks & 1) * 8;  // as write_act
    const f32x2 s01{ldexpf(s_stem.x, -ex), ldexpf(s_stem.y, -ex)}, s23{ldexpf(s_stem.z, -ex), ldexpf(s_stem.w, -ex)};
    const f32x2 b01{b_stem.x, b_stem.y}, b23{b_stem.z, b_stem.w};
    const float up = ldexpf(1.0f, ex_out);
    float mx = 0.0f;
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      f32x2 y01 = pk_fma(f32x2{acc[g][0], acc[g][1]}, s01, b01);
      f32x2 y23 = pk_fma(f32x2{acc[g][2], acc[g][3]}, s23, b23);
      y01 = f32x2{max_bits(y01.x, 0), max_bits(y01.y, 0)};
      y23 = f32x2{max_bits(y23.x, 0), max_bits(y23.y, 0)};
      if (is_valid(g)) mx = max3_abs(max3_abs(mx, y01.x, y01.y), y23.x, y23.y);
      x0[g] = f32x4{y01.x, y01.y, y23.x, y23.y};
      unsigned h0, h1, l0, l1;
      split2(y01.x * up, y01.y * up, h0, l0);
      split2(y23.x * up, y23.y * up, h1, l1);
      if (is_valid(g)) {
        *reinterpret_cast<u32x2*>(wbase + slot_b(g)) = u32x2{h0, h1};
        *reinterpret_cast<u32x2*>(wbase + slot_b(g) + PL) = u32x2{l0, l1};
      }
    }
#pragma unroll
    for (int g = X0L; g < NG; ++g) asm volatile("" : "+a"(x0[g]));
    post_max(mx, 0);
    LNSTAMP(34, __builtin_amdgcn_s_memtime());
    __syncthreads();  // the grid and the maxima are written; every wave is done with the stem's input planes
    LNSTAMP(35, __builtin_amdgcn_s_memtime());
#pragma unroll
    for (int g = 0; g < X0L; ++g) {
      x0s[g * kLnThreads + tid] = x0[g];
      x0[g] = f32x4{0.f, 0.f, 0.f, 0.f};  // not kept in registers
    }
    max_in = board_max(0);
    ex = ex_out;
  } else {
    const int ex_out = out_exp(0, max_obs);
#pragma unroll
    for (int g = 0; g < NG; ++g) x0[g] = f32x4{0.f, 0.f, 0.f, 0.f};
    // the stem output itself is kept (unscaled) for the tower's final residual
    const float mx = epilogue(s_stem, b_stem, true, false, x0, false, 0);
#pragma unroll
    for (int g = 0; g < NG; ++g) x0[g] = acc[g];
    const float up = ldexpf(1.0f, ex_out);
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      unsigned h0, h1, l0, l1;
      split2(x0[g][0] * up, x0[g][1] * up, h0, l0);
      split2(x0[g][2] * up, x0[g][3] * up, h1, l1);
      acc[g] = f32x4{__builtin_bit_cast(float, h0), __builtin_bit_cast(float, h1), __builtin_bit_cast(float, l0),
                     __builtin_bit_cast(float, l1)};
    }
    // x0 waits out the tower in AGPRs (read once, by the last conv): its VGPRs go to the loop
#pragma unroll
    for (int g = X0L; g < NG; ++g) asm volatile("" : "+a"(x0[g]));
    post_max(mx, 0);
    LNSTAMP(34, __builtin_amdgcn_s_memtime());
    __syncthreads();  // every wave is done with the stem's input planes (the x0 stash reuses them)
    LNSTAMP(35, __builtin_amdgcn_s_memtime());
    write_act();
#pragma unroll
    for (int g = 0; g < X0L; ++g) {
      x0s[g * kLnThreads + tid] = x0[g];
      x0[g] = f32x4{0.f, 0.f, 0.f, 0.f};  // not kept in registers
    }
    __syncthreads();
    max_in = board_max(0);
    ex = ex_out;
  }
  LNSTAMP(3, __builtin_amdgcn_s_memtime());

  // ---- residual tower: nlayers convs 64 -> 64; ReLU after each block's first conv; the last
  // adds x0 and takes the ReLU (x = relu(x + res_blocks(x)), blokus_nnet.py:140-141)
  for (int layer = 0; layer < nlayers; ++layer) {
    const bool more = layer + 1 < nlayers;
    // the layer's output scale and bias (folded BN) are loaded here, under the MFMA loop
    const f32x4 sv = *reinterpret_cast<const f32x4*>(st + layer * 64 + oc);
    const f32x4 bv = *reinterpret_cast<const f32x4*>(bt + layer * 64 + oc);
    // the next conv's output bound (bounds holds the stem and every tower conv: always in range)
    const float bnd_a = bounds[2 * (layer + 1)], bnd_b = bounds[2 * (layer + 1) + 1];
    // chunk c = (tap c/2, channel half c%2): the lane's octet 4 (c%2) + ks has its hi plane at
    // ks*4 + 2 (c%2) (lo next to it), so from ab the offset is a compile-time immediate < 2^16
    auto coff_of = [&](int c) {
      const int t = c >> 1;
      return 2 * (c & 1) * PL + ((t / 3 - 1) * RS + (t % 3 - 1)) * 16 + kBias;
    };
    ln_prime<NG, PL>(rb, act, ab, coff_of(0));
    if (layer == 1) LNSTAMP(26, __builtin_amdgcn_s_memtime());
    if constexpr (EDGE) {
      // the chunk index as a compile-time value: each chunk takes its own list of active groups
      // (the weight ring as in the loop below)
      ln_each_chunk(
          [&](auto cc) __attribute__((always_inline)) {
            constexpr int c = decltype(cc)::value, cn = c + kLnWpf, sn = cn % (kLnWpf + 1);
            using S = LnEdgeSched<N>;
            if (layer == 1 && c == 1) LNSTAMP(27, __builtin_amdgcn_s_memtime());
            if (layer == 1 && c == 9) LNSTAMP(28, __builtin_amdgcn_s_memtime());
            const int wl = cn < 18 || more ? layer + cn / 18 : layer;
            wq[sn][0] = wload(wl, cn % 18, 0);
            wq[sn][1] = wload(wl, cn % 18, 1);
            const h16x8* w = wq[c % (kLnWpf + 1)];
            ln_chunk_il_act<NG, S::active(c), S::first(c), S::pos0(c), PL>(acc, w[0], w[1], act, ab, coff_of(c),
                                                                         coff_of(c + 1 < 18 ? c + 1 : c), rb);
          },
          std::make_integer_sequence<int, 18>{});
    } else {
#pragma unroll
      for (int c = 0; c < 18; ++c) {
        if (layer == 1 && c == 1) LNSTAMP(27, __builtin_amdgcn_s_memtime());
        if (layer == 1 && c == 9) LNSTAMP(28, __builtin_amdgcn_s_memtime());
        const int cn = c + kLnWpf, sn = cn % (kLnWpf + 1);
        if (cn < 18) {
          wq[sn][0] = wload(layer, cn, 0);
          wq[sn][1] = wload(layer, cn, 1);
        } else {  // the next layer's first chunks; the last layer reloads its own (never used): an
                  // unconditional load keeps the wait count static (a branch made it vmcnt(0), an
                  // exposed L2 round trip per layer)
          const int nl = more ? layer + 1 : layer;
          wq[sn][0] = wload(nl, cn - 18, 0);
          wq[sn][1] = wload(nl, cn - 18, 1);
        }
        const h16x8* w = wq[c % (kLnWpf + 1)];
        if (c == 0)
          ln_chunk_il<NG, true, PL>(acc, w[0], w[1], act, ab, coff_of(0), coff_of(1), rb);
        else
          ln_chunk_il<NG, false, PL>(acc, w[0], w[1], act, ab, coff_of(c), coff_of(c + 1 < 18 ? c + 1 : c), rb);
      }
    }
    // the last chunk's read-ahead (ln_chunk_il: untracked) lands before its registers are reused
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    ln_mfma_drain(acc);
    if (layer < 8) LNSTAMP(4 + 2 * layer, __builtin_amdgcn_s_memtime());
    const bool last = layer + 1 == nlayers;
    if (!last) {
      const int ex_out = scale_exp(bnd_a * max_in + bnd_b);  // = out_exp(layer + 1, max_in)
      if (layer == 1) LNSTAMP(21, __builtin_amdgcn_s_memtime());
      __syncthreads();  // every wave has finished reading the grid: the outputs go in place as made
      if (layer == 1) LNSTAMP(22, __builtin_amdgcn_s_memtime());
      const float mx = epilogue(sv, bv, !(layer & 1), false, x0, true, ex_out, true);
      if (layer == 1) LNSTAMP(23, __builtin_amdgcn_s_memtime());
      post_max(mx, (layer + 1) & 1);
      if (layer == 1) LNSTAMP(24, __builtin_amdgcn_s_memtime());
      __syncthreads();
      if (layer == 1) LNSTAMP(25, __builtin_amdgcn_s_memtime());
      max_in = board_max((layer + 1) & 1);
      ex = ex_out;
    } else {
#pragma unroll
      for (int g = 0; g < X0L; ++g) x0[g] = x0s[g * kLnThreads + tid];
      epilogue(sv, bv, true, true, x0, false, 0);
    }
    if (layer < 8) LNSTAMP(5 + 2 * layer, __builtin_amdgcn_s_memtime());
  }

  // ---- outputs: the tower output (optional) and the heads (blokus_nnet.py:146-150, BN folded)
  f32x4 hw0, hw1, hwv;  // FAST: the 1x1 heads' weights, in flight across the barrier below
  if constexpr (FAST) {
    hw0 = *reinterpret_cast<const f32x4*>(hd.wp + oc);
    hw1 = *reinterpret_cast<const f32x4*>(hd.wp + 64 + oc);
    hwv = *reinterpret_cast<const f32x4*>(hd.wv + oc);
  }
  if (xout) {
#pragma unroll
    for (int g = 0; g < NG; ++g)
      if (is_valid(g))
        *reinterpret_cast<f32x4*>(xout + (b * NN + ln_pixel<N>(slot_b(g) / 16)) * 64 + oc) = acc[g];
  }
  LNSTAMP(37, __builtin_amdgcn_s_memtime());
  __syncthreads();  // every wave is done with the activation grid: the heads' scratch reuses it
  if constexpr (FAST) {
    // The heads' scratch: hs[wave][grid slot][4] = the wave's 16-channel sums {policy 0, policy 1,
    // value, -} of the pixel at that slot (16 B per entry: one store per lane, consecutive slots in
    // consecutive bank groups), then vfeat and part. Four groups are reduced at a time
    // (ln_quad_sum): k-group row r of the lanes ends with the sums of group g0 + r (the last
    // group again past the end: the same values to the same place), so every lane stores.
    constexpr int SL = (N + 2) * RS, Q = NN / 4;
    static_assert(NN % 4 == 0, "k_leafnet_x3: quarters of the value-MLP inputs");
    static_assert(4 * SL * 16 + (NN + 4 * 64) * 4 <= 16 * PL, "k_leafnet_x3: the heads' scratch fits the activation planes");
    unsigned char* hb = act + wave * (SL * 16);
    const f32x2 wx{hw0.x, hw1.x}, wy{hw0.y, hw1.y}, wz{hw0.z, hw1.z}, ww{hw0.w, hw1.w};
#pragma unroll
    for (int g0 = 0; g0 < NG; g0 += 4) {
      f32x2 p[4];
      float q[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const f32x4 y = acc[g0 + r < NG ? g0 + r : NG - 1];
        p[r] = ln_dot2(y, wx, wy, wz, ww);
        q[r] = y.x * hwv.x + y.y * hwv.y + y.z * hwv.z + y.w * hwv.w;
      }
      const float d0 = ln_quad_sum(p[0].x, p[1].x, p[2].x, p[3].x);
      const float d1 = ln_quad_sum(p[0].y, p[1].y, p[2].y, p[3].y);
      const float d2 = ln_quad_sum(q[0], q[1], q[2], q[3]);
      int sl = slot_b(g0);
      bool ok = is_valid(g0);
#pragma unroll
      for (int r = 1; r < 4; ++r) {
        const int g = g0 + r < NG ? g0 + r : NG - 1;
        sl = ks == r ? slot_b(g) : sl;
        ok = ks == r ? (bool)is_valid(g) : ok;
      }
      if (ok) *reinterpret_cast<f32x4*>(hb + sl) = f32x4{d0, d1, d2, 0.0f};
    }
    // every global load of the phases below is issued here, ahead of the barriers and of the pf
    // stores (which the compiler cannot rule out as aliases): the head biases, the wave's quarter
    // of W1 (L2-resident), and wave 0's W2 rows, b2 and b1
    const float bp0 = hd.bp[0], bp1 = hd.bp[1], bv0 = hd.bv[0];
    const int q0 = Q * wave;
    // (as buffer loads with immediate row offsets the Q loads took ~1k cycles longer: measured, dropped)
    float w[Q];
#pragma unroll
    for (int k = 0; k < Q; ++k) w[k] = hd.w1t[(size_t)(q0 + k) * 64 + l];
    float w2[kMaxP], b2[kMaxP], b1 = 0.0f;
#pragma unroll
    for (int q = 0; q < kMaxP; ++q) w2[q] = b2[q] = 0.0f;
    if (wave == 0) {
#pragma unroll
      for (int q = 0; q < kMaxP; ++q) {
        w2[q] = q < hd.P ? hd.w2[q * 64 + l] : 0.0f;
        b2[q] = q < hd.P ? hd.b2[q] : 0.0f;
      }
      b1 = hd.b1[l];
    }
    __syncthreads();
    LNSTAMP(20, __builtin_amdgcn_s_memtime());
    // pf = relu(policy 1x1 conv + bp) (channel-major), vfeat = relu(value 1x1 conv + bv): the
    // waves' sums added as ((w0 + w1) + w2) + w3
    float* vfeat = reinterpret_cast<float*>(act + 4 * SL * 16);
    float* part = vfeat + NN;
    for (int i = tid; i < NN; i += kLnThreads) {
      const unsigned char* q = act + ((i / N + 1) * RS + i % N + 1) * 16;
      const f32x4 a0 = *reinterpret_cast<const f32x4*>(q), a1 = *reinterpret_cast<const f32x4*>(q + SL * 16),
                  a2 = *reinterpret_cast<const f32x4*>(q + 2 * SL * 16), a3 = *reinterpret_cast<const f32x4*>(q + 3 * SL * 16);
      const float p0 = ((a0.x + a1.x) + a2.x) + a3.x, p1 = ((a0.y + a1.y) + a2.y) + a3.y,
                  pv = ((a0.z + a1.z) + a2.z) + a3.z;
      hd.pf[b * 2 * NN + i] = fmaxf(p0 + bp0, 0.0f);
      hd.pf[b * 2 * NN + NN + i] = fmaxf(p1 + bp1, 0.0f);
      vfeat[i] = fmaxf(pv + bv0, 0.0f);
    }
    __syncthreads();
    LNSTAMP(38, __builtin_amdgcn_s_memtime());
    {
      // v = tanh(W2 relu(W1 vfeat + b1) + b2); wave w: inputs [Q w, Q (w + 1)) of W1, its vfeat
      // quarter read 16 B at a time where the quarters are 16-B aligned; the sums in the order of
      // the other code (a0 even, a1 odd inputs in blocks of 10, the rest into a0)
      float vf[Q];
      if constexpr (Q % 4 == 0) {
#pragma unroll
        for (int k = 0; k < Q; k += 4) {
          const f32x4 t = *reinterpret_cast<const f32x4*>(vfeat + q0 + k);
          vf[k] = t.x;
          vf[k + 1] = t.y;
          vf[k + 2] = t.z;
          vf[k + 3] = t.w;
        }
      } else {
#pragma unroll
        for (int k = 0; k < Q; ++k) vf[k] = vfeat[q0 + k];
      }
      float a0 = 0.f, a1 = 0.f;
      int k = 0;
#pragma unroll
      for (; k + 10 <= Q; k += 10) {
#pragma unroll
        for (int u = 0; u < 10; u += 2) {
          a0 += w[k + u] * vf[k + u];
          a1 += w[k + u + 1] * vf[k + u + 1];
        }
      }
#pragma unroll
      for (; k < Q; ++k) a0 += w[k] * vf[k];
      part[wave * 64 + l] = a0 + a1;
    }
    __syncthreads();
    LNSTAMP(39, __builtin_amdgcn_s_memtime());
    if (wave == 0) {
      const float h = fmaxf(((part[l] + part[64 + l]) + (part[128 + l] + part[192 + l])) + b1, 0.0f);
      // every output's sum first, then one tanh: lane q takes output q's sum and bias and stores it
      float x = 0.0f;
#pragma unroll
      for (int q = 0; q < kMaxP; ++q) {
        if (q < hd.P) {
          const float sq = wave_sum_f(w2[q] * h) + b2[q];
          x = l == q ? sq : x;
        }
      }
      const float t = tanhf(x);
      if (l < hd.P) hd.v[b * hd.P + l] = t;
    }
  } else {
    float* hp = reinterpret_cast<float*>(act);  // [NN][4 waves][3]
    {
      const f32x4 wp0 = *reinterpret_cast<const f32x4*>(hd.wp + oc);
      const f32x4 wp1 = *reinterpret_cast<const f32x4*>(hd.wp + 64 + oc);
      const f32x4 wvv = *reinterpret_cast<const f32x4*>(hd.wv + oc);
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        const f32x4 y = acc[g];
        float d[3];
        const f32x4* w[3] = {&wp0, &wp1, &wvv};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          // the sum over the 4 k-groups: a + a(lane ^ 16), then + (lane ^ 32), as two VALU swaps
          // (v_permlane16/32_swap) instead of LDS permutes; x + y is the same sum in either order
          const float a = y.x * (*w[k]).x + y.y * (*w[k]).y + y.z * (*w[k]).z + y.w * (*w[k]).w;
          const auto s16 = __builtin_amdgcn_permlane16_swap(__float_as_uint(a), __float_as_uint(a), false, false);
          const float a16 = __uint_as_float(s16[0]) + __uint_as_float(s16[1]);
          const auto s32 = __builtin_amdgcn_permlane32_swap(__float_as_uint(a16), __float_as_uint(a16), false, false);
          d[k] = __uint_as_float(s32[0]) + __uint_as_float(s32[1]);
        }
        if (ks == 0 && is_valid(g)) {
          float* dst = hp + (ln_pixel<N>(slot_b(g) / 16) * 4 + wave) * 3;
          dst[0] = d[0];
          dst[1] = d[1];
          dst[2] = d[2];
        }
      }
    }
    __syncthreads();
    LNSTAMP(20, __builtin_amdgcn_s_memtime());
    // pf = relu(policy 1x1 conv + bp) (channel-major), vfeat = relu(value 1x1 conv + bv), then
    // v = tanh(W2 relu(W1 vfeat + b1) + b2); the 4 waves sweep quarters of W1's inputs
    float* vfeat = hp + NN * 12;
    float* part = vfeat + NN;
    // the head biases in registers first: read inside the loop, each was re-loaded after every pf
    // store (the compiler cannot rule out aliasing), one dependent round trip per store
    const float bp0 = hd.bp[0], bp1 = hd.bp[1], bv0 = hd.bv[0];
    for (int i = tid; i < NN; i += kLnThreads) {
      const float* q = hp + i * 12;
      const float p0 = ((q[0] + q[3]) + q[6]) + q[9], p1 = ((q[1] + q[4]) + q[7]) + q[10],
                  pv = ((q[2] + q[5]) + q[8]) + q[11];
      hd.pf[b * 2 * NN + i] = fmaxf(p0 + bp0, 0.0f);
      hd.pf[b * 2 * NN + NN + i] = fmaxf(p1 + bp1, 0.0f);
      vfeat[i] = fmaxf(pv + bv0, 0.0f);
    }
    __syncthreads();
    LNSTAMP(38, __builtin_amdgcn_s_memtime());
    {
      // wave w: inputs [Q w, Q (w + 1)) of W1 (L2-resident), every load issued before the first FMA
      constexpr int Q = NN / 4;
      static_assert(NN % 4 == 0, "k_leafnet_x3: quarters of the value-MLP inputs");
      const int q0 = Q * wave;
      float w[Q];
#pragma unroll
      for (int k = 0; k < Q; ++k) w[k] = hd.w1t[(size_t)(q0 + k) * 64 + l];
      float a0 = 0.f, a1 = 0.f;
      int k = 0;
#pragma unroll
      for (; k + 10 <= Q; k += 10) {
#pragma unroll
        for (int u = 0; u < 10; u += 2) {
          a0 += w[k + u] * vfeat[q0 + k + u];
          a1 += w[k + u + 1] * vfeat[q0 + k + u + 1];
        }
      }
#pragma unroll
      for (; k < Q; ++k) a0 += w[k] * vfeat[q0 + k];
      part[wave * 64 + l] = a0 + a1;
    }
    __syncthreads();
    LNSTAMP(39, __builtin_amdgcn_s_memtime());
    if (wave == 0) {
      // W2 rows and b2 loaded together before the value stores (same aliasing as above)
      float w2[kMaxP], b2[kMaxP];
#pragma unroll
      for (int q = 0; q < kMaxP; ++q) {
        w2[q] = q < hd.P ? hd.w2[q * 64 + l] : 0.0f;
        b2[q] = q < hd.P ? hd.b2[q] : 0.0f;
      }
      const float h = fmaxf(((part[l] + part[64 + l]) + (part[128 + l] + part[192 + l])) + hd.b1[l], 0.0f);
#pragma unroll
      for (int q = 0; q < kMaxP; ++q) {
        if (q < hd.P) {
          const float sum = wave_sum_f(w2[q] * h);
          if (l == 0) hd.v[b * hd.P + q] = tanhf(sum + b2[q]);
        }
      }
    }
  }
  LNSTAMP(29, __builtin_amdgcn_s_memtime());
  LNSTAMP(31, __builtin_amdgcn_s_memrealtime());
}

static_assert(ln_lds_bytes(20) <= 160 * 1024, "k_leafnet_x3<20>: LDS");
static_assert(ln_edge_map_is_bijection<20>(), "LnEdgePixMap<20>: every board pixel in exactly one MFMA column");
static_assert(ln_edge_sched_skips_only_halo<20>(), "LnEdgeSched<20>: a skipped (group, chunk) reads only the halo");
static_assert(LnEdgeSched<20>::pos0(18) == 18 * 25 - 24, "LnEdgeSched<20>: 24 of 450 pairs left out");

// BK_LN_EDGE (default 1): the 20x20 board on the edge schedule (0: the full schedule on
// LnPixMap); read per launch, so one build compares the two (a captured graph keeps what it read)
bool ln_edge() {
  const char* e = getenv("BK_LN_EDGE");
  return e ? atoi(e) != 0 : true;
}

// BK_LN_FAST (default 1): the FAST instantiations (0: the others, the code as it was before them);
// read per launch like BK_LN_EDGE
bool ln_fast() {
  const char* e = getenv("BK_LN_FAST");
  return e ? atoi(e) != 0 : true;
}

// The refusals shared by bk_leafnet_x3_run and (per table entry, rows_form) bk_leafnet_x3_rows,
// as "<who>: <what>": null operands, the N / P / np rules of the kernel family a.np names, the
// depth and the alignments. out: bk_leafnet_x3_run's tower output (may be null). The rows form
// runs one board per workgroup, so it does not look at np's boards_per_wg.
int ln_check(const bk_leafnet_args& a, const char* who, const float* out, bool rows_form) {
  const auto a4 = [](const void* p) { return ((uintptr_t)p & 3u) == 0; };
  const auto a16 = [](const void* p) { return ((uintptr_t)p & 15u) == 0; };
  const bool np = a.np != 0;
  const char* bad = nullptr;
  if (!a.obs == !a.states)
    bad = "exactly one of obs and states must be set";
  else if (!(a.wstem && a.sstem && a.bstem && a.wtower && a.stower && a.btower && a.bounds && a.wp && a.bp && a.wv &&
             a.bv && a.w1t && a.b1 && a.w2 && a.b2 && a.pf && a.vout && a.P > 0))
    bad = "null net operand";
  else if (np && !(a.N == 7 || a.N == 14 || a.N == 20))
    bad = "N must be 7, 14 or 20 (np form)";
  else if (np && !(a.P >= 2 && a.P <= kMaxP))
    bad = "P must be 2, 3 or 4 (np form)";
  else if (np && !rows_form && !(a.np == 1 || a.np == 2 || (a.np == 5 && a.N == 7)))
    bad = "np must be 0 or boards_per_wg + 1, boards_per_wg 0, 1 or (N = 7 only) 4";
  // the classic planar form takes 8 planes whatever P: P reaches only the value head there
  else if (!np && a.states && a.P != kLnP)
    bad = "P must be 4 (the stem takes 8 observation planes; np = 0)";
  else if (!np && !(a.N == 14 || a.N == 20))
    bad = "N must be 14 or 20 (np = 0)";
  else if (a.nlayers < 1)
    bad = "at least one tower conv";
  else if (a.states && !a4(a.states))
    bad = "states must be 4-byte aligned";
  else if (np && a.obs && !a4(a.obs))
    bad = "obs must be 4-byte aligned";
  else if (!(a16(a.wstem) && a16(a.wtower) && a16(a.sstem) && a16(a.bstem) && a16(a.stower) && a16(a.btower) &&
             a16(a.wp) && a16(a.wv) && a16(out)))
    bad = "16-byte aligned buffers";
  if (!bad) return BK_OK;
  set_error(std::string(who) + ": " + bad);
  return BK_EINVAL;
}

// One launch of k_leafnet_x3 on `grid` workgroups: the weight set w, rows t0.. of a's outputs and
// of the whole-batch tower output `out` (may be null). The rows form passes an empty w and
// t0 = 0: the kernel takes each row's tree and weights from the table in `in`.
template <typename In>  // const float* (the planes of row t0), LnStates (at row t0) or LnRows
int ln_launch(In in, int grid, const bk_leafnet_args& a, const LnNet& w, int t0, float* out, void* stream) {
  const void* fns[6] = {(const void*)k_leafnet_x3<14, In>,       (const void*)k_leafnet_x3<20, In>,
                        (const void*)k_leafnet_x3<20, In, true>, (const void*)k_leafnet_x3<14, In, false, true>,
                        (const void*)k_leafnet_x3<20, In, false, true>, (const void*)k_leafnet_x3<20, In, true, true>};
  if (set_max_dynamic_lds(fns, 6, ln_lds_bytes(20)) != BK_OK) return BK_EHIP;
  const LnHeads h = ln_heads_of(a, w, t0);
  float* xout = out ? out + (size_t)t0 * a.N * a.N * 64 : nullptr;
  const dim3 g(grid), b(kLnThreads);
  hipStream_t s = (hipStream_t)stream;
  const int which = (a.N == 20 ? (ln_edge() ? 2 : 1) : 0) + (ln_fast() ? 3 : 0);
  void* args[] = {(void*)&in,   (void*)&w.wstem,   (void*)&w.sstem,   (void*)&w.bstem, (void*)&w.wt, (void*)&w.st,
                  (void*)&w.bt, (void*)&w.bounds, (void*)&a.nlayers, (void*)&h,       (void*)&xout};
  (void)hipLaunchKernel(fns[which], g, b, args, ln_lds_bytes(a.N == 20 ? 20 : 14), s);
  return launch_check(std::is_same<In, LnRows>::value     ? "k_leafnet_x3 (rows)"
                      : std::is_same<In, LnStates>::value ? "k_leafnet_x3 (states)"
                                                          : "k_leafnet_x3");
}

}  // namespace
}  // namespace bk

using namespace bk;

extern "C" {

int bk_leafnet_x3_weight_bytes(int cin) {
  return cin == 64 || cin == 8 ? ln_chunks(cin) * 4 * 2 * kBlock * 2 : -1;
}

int bk_leafnet_x3_supported(int N) { return N == 14 || N == 20; }

#if BK_LN_STAMP
int bk_ln_stamps(unsigned long long* out) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_ln_stamps), sizeof(g_ln_stamps)) == hipSuccess ? 0 : -1;
}
int bk_ln_stamps_clear() {
  static unsigned long long zeros[256 * 4 * kLnStamps];
  return hipMemcpyToSymbol(HIP_SYMBOL(g_ln_stamps), zeros, sizeof(zeros)) == hipSuccess ? 0 : -1;
}
#endif

int bk_ln_path_counts(int enable, unsigned* counts) {
  unsigned cur[3];
  if (hipMemcpyFromSymbol(cur, HIP_SYMBOL(g_ln_paths), sizeof(cur)) != hipSuccess) return BK_EHIP;
  if (counts) {
    counts[0] = cur[1];
    counts[1] = cur[2];
  }
  const unsigned next[3] = {enable ? 1u : 0u, 0u, 0u};
  return hipMemcpyToSymbol(HIP_SYMBOL(g_ln_paths), next, sizeof(next)) == hipSuccess ? BK_OK : BK_EHIP;
}

int bk_leafnet_x3_run(const bk_leafnet_args* a, int t0, int n, float* out, void* stream) {
  BK_REQUIRE(a && t0 >= 0 && n >= 0, "bk_leafnet_x3_run: bad argument");
  if (int rc = ln_check(*a, "bk_leafnet_x3_run", out, false)) return rc;
  if (n == 0) return BK_OK;
  if (a->np) return leafnet_np_run(a, 1, nullptr, 0, t0, n, out, stream);
  const LnNet w = ln_net_of(*a);
  if (a->obs) return ln_launch(a->obs + (size_t)t0 * kStemCinX3 * a->N * a->N, n, *a, w, t0, out, stream);
  return ln_launch(ln_states_of<LnStates>(*a, t0), n, *a, w, t0, out, stream);
}

// The four positional entries: wrappers that fill the struct and run rows [0, B).
int bk_leafnet_x3(const float* obs, int B, int N, int cin, const void* wstem, const float* sstem, const float* bstem,
                  int nlayers, const void* wtower, const float* stower, const float* btower, const float* bounds,
                  const float* wp,
                  const float* bp, const float* wv, const float* bv, const float* w1t, const float* b1,
                  const float* w2, const float* b2, int P, float* pf, float* vout, float* out, void* stream) {
  BK_REQUIRE(cin == kStemCinX3, "bk_leafnet_x3: the stem takes 8 observation planes");
  const bk_leafnet_args a{obs, nullptr, nullptr, N,  P,  nlayers, wstem, sstem, bstem, wtower, stower, btower,
                          bounds, wp,   bp,      wv, bv, w1t,     b1,    w2,    b2,    pf,     vout,   0};
  return bk_leafnet_x3_run(&a, 0, B, out, stream);
}

int bk_leafnet_x3_states(const void* states, const int32_t* status, int B, int N, int P, const void* wstem,
                         const float* sstem, const float* bstem, int nlayers, const void* wtower,
                         const float* stower, const float* btower, const float* bounds, const float* wp,
                         const float* bp, const float* wv, const float* bv, const float* w1t, const float* b1,
                         const float* w2, const float* b2, float* pf, float* vout, float* out, void* stream) {
  const bk_leafnet_args a{nullptr, states, status, N,  P,  nlayers, wstem, sstem, bstem, wtower, stower, btower,
                          bounds,  wp,     bp,     wv, bv, w1t,     b1,    w2,    b2,    pf,     vout,   0};
  return bk_leafnet_x3_run(&a, 0, B, out, stream);
}

int bk_leafnet_x3_rows(const bk_leafnet_args* nets, int nnets, const bk_arena_rows* rows, int sim, void* stream) {
  BK_REQUIRE(rows && nnets >= 0 && nnets <= kLnMaxNets && sim >= 0, "bk_leafnet_x3_rows: bad argument");
  BK_REQUIRE(rows->R >= 0 && rows->T >= 0 && (rows->R == 0 || (rows->tree_of_row && rows->net_of_row && rows->sims_of_row)),
             "bk_leafnet_x3_rows: bad row tables");
  if (nnets == 0 || rows->R == 0) return BK_OK;
  BK_REQUIRE(nets, "bk_leafnet_x3_rows: null net table");
  const bk_leafnet_args& a0 = nets[0];
  for (int k = 0; k < nnets; ++k) {
    const bk_leafnet_args& a = nets[k];
    BK_REQUIRE(!a.obs && a.states && a.status, "bk_leafnet_x3_rows: states form only (states and status set, obs null)");
    BK_REQUIRE(a.states == a0.states && a.status == a0.status && a.pf == a0.pf && a.vout == a0.vout && a.N == a0.N &&
                   a.P == a0.P && a.nlayers == a0.nlayers && a.np == a0.np,
               "bk_leafnet_x3_rows: the nets must share states, status, pf, vout, N, P, nlayers and np");
    if (int rc = ln_check(a, "bk_leafnet_x3_rows", nullptr, true)) return rc;
  }
  if (a0.np) return leafnet_np_run(nets, nnets, rows, sim, 0, rows->R, nullptr, stream);
  return ln_launch(ln_rows_of(nets, nnets, rows, sim), rows->R, a0, LnNet{}, 0, nullptr, stream);
}

}  // extern "C"

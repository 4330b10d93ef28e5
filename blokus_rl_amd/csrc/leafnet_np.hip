// leafnet_np.hip — k_leafnet_x3 (leafnet.hip) for the other board shapes: any player count P (the
// stem's 2P observation planes zero-padded to 8 channels) on 7x7, 14x14 and 20x20 boards, and at
// 7x7 four boards per workgroup (Q = 4) besides one (Q = 1).
//
// Same arithmetic as leafnet.hip: split-f16 products on v_mfma_f32_16x16x32_f16, the layer input
// in LDS as zero-haloed grids of 16-B slots (16 planes + 2 for the stem), the accumulators of all
// NG pixel groups resident for a layer, the K loop of leafnet_common.h (ln_chunk*). What differs:
//  * the grid (NpGeo). Q = 4 packs four 7x7 boards as 2 x 2 into one grid of 17 rows x 18 slots
//    with shared zero separator rows and columns (rows / columns 0, 8, 16): a tap that leaves a
//    board reads a separator, exactly the halo it would read alone. 196 pixels = 13 groups (15
//    with the ring padding), as many as one 14x14 board: each A fragment streamed from L2 feeds
//    four boards' MFMAs.
//  * the activation scale 2^ex stays per board. 49 is no multiple of 16, so some group's 16
//    columns must mix boards: the pixel map (NpPixMap) gives groups 3q..3q+2 to board q alone and
//    puts the four 49th pixels into group 12, the one group whose epilogue takes the (ex, ex_out)
//    of its column's board per lane; the maxima are reduced per board. The columns of an MFMA
//    are independent and the K order is the same, so a board's pf, v and tower output are
//    bitwise those of Q = 1, whatever its neighbours, its place in the workgroup and the batch.
//  * P is a kernel argument: the planar form reads 2P planes and zero-fills channels 2P..7, the
//    states form reads P planes of row words; to_move < P selects the mover plane.
//  * the value MLP's first layer is partitioned for any N*N (below, "heads").
#include "../../include/blokus_engine.h"
#include "ctx.h"

#include <type_traits>

#define BK_LN_VACC 1
#include "leafnet_common.h"

namespace bk {
namespace {

struct NpStates {
  const uint32_t* states;
  const int32_t* status;
};

// The grid of Q boards (1, or 4 as 2 x 2) of N x N pixels. Pixel p of the workgroup = board
// p / NN, cell p % NN; slot = grid row * RS + grid column, in 16-B units.
template <int N, int Q>
struct NpGeo {
  static_assert(Q == 1 || (Q == 4 && N == 7), "four boards per workgroup: 7x7 only");
  static constexpr int QS = Q == 4 ? 2 : 1;         // boards per grid side
  static constexpr int NN = N * N, NPIX = Q * NN;
  static constexpr int SPAN = QS * (N + 1) - 1;     // pixel rows / columns with the separators between boards
  static constexpr int GR = SPAN + 2;               // grid rows
  // slot classes mod 16 balanced (bank conflicts of the B reads): 18 for the 2 x 2 grid as for 14x14
  static constexpr int RS = Q == 4 ? 18 : (N == 7 ? 9 : ln_row(N));
  static constexpr int PL = (GR * RS * 16 + 255) / 256 * 256;
  static constexpr int NG = ((NPIX + 15) / 16 + kLnSlots - 1) / kLnSlots * kLnSlots;
  static constexpr int X0L = ln_x0_lds_groups(N);   // stem output groups that wait in LDS (20x20)
  static constexpr int kStash = 2 * PL > X0L * 256 * 16 ? 2 * PL : X0L * 256 * 16;
  static constexpr int kLdsBody = 16 * PL + kStash;
  static constexpr int kLds = kLdsBody + 256;       // + the wave maxima
  static_assert(RS >= SPAN + 2 && SPAN + 2 <= GR, "NpGeo: halo");
  static_assert(16 * PL >= (NPIX * 13 + Q * 256) * 4, "NpGeo: the heads' scratch reuses the activation planes");
  static __host__ __device__ constexpr int slot_of(int p) {
    const int q = p / NN, r = p % NN / N, c = p % N;
    return (1 + (q / QS) * (N + 1) + r) * RS + 1 + (q % QS) * (N + 1) + c;
  }
  static __host__ __device__ constexpr bool is_pixel(int slot) {
    const int rr = slot / RS - 1, cc = slot % RS - 1;
    return rr >= 0 && cc >= 0 && rr < SPAN && cc < SPAN && rr % (N + 1) != N && cc % (N + 1) != N;
  }
};

// LnPixMap over NpGeo's pixels: MFMA column (g, n) -> grid slot, one pixel per slot class mod 16
// per group where the classes allow, leftovers in the gaps, -1 for a spare column.
template <int N, int Q>
struct NpPixMap {
  using G = NpGeo<N, Q>;
  int slot[G::NG * 16];
  constexpr NpPixMap() : slot() {
    bool used[G::NPIX] = {};
    for (int i = 0; i < G::NG * 16; ++i) slot[i] = -1;
    if constexpr (Q == 4) {
      // groups 3q..3q+2 hold 48 pixels of board q alone (so their columns' board, and with it the
      // activation scale, is a compile-time property of the group); group 12 holds the boards'
      // 49th pixels in columns 0..3 (column j: board j), the only group that mixes boards
      for (int q = 0; q < Q; ++q) {
        for (int g = 3 * q; g < 3 * q + 3; ++g)
          for (int r = 0; r < 16; ++r)
            for (int p = q * G::NN; p < (q + 1) * G::NN; ++p) {
              const int sl = G::slot_of(p);
              if (!used[p] && sl % 16 == r) {
                used[p] = true;
                slot[g * 16 + r] = sl;
                break;
              }
            }
        int p = q * G::NN;
        for (int i = 3 * q * 16; i < (3 * q + 3) * 16; ++i) {
          if (slot[i] >= 0) continue;
          while (used[p]) ++p;
          used[p] = true;
          slot[i] = G::slot_of(p);
        }
        while (used[p]) ++p;
        slot[12 * 16 + q] = G::slot_of(p);
      }
      return;
    }
    for (int g = 0; g < G::NG; ++g)
      for (int r = 0; r < 16; ++r)
        for (int p = 0; p < G::NPIX; ++p) {
          const int sl = G::slot_of(p);
          if (!used[p] && sl % 16 == r) {
            used[p] = true;
            slot[g * 16 + r] = sl;
            break;
          }
        }
    int p = 0;
    for (int i = 0; i < G::NG * 16; ++i) {
      if (slot[i] >= 0) continue;
      while (p < G::NPIX && used[p]) ++p;
      if (p == G::NPIX) break;
      used[p] = true;
      slot[i] = G::slot_of(p);
    }
  }
};
template <int N, int Q>
__device__ constexpr NpPixMap<N, Q> kNpPixMap{};

constexpr int kNpRowStride = kMaxP * kMaxN + 1;  // a board's staged row words, to_move last

template <int N, int Q, typename In>  // In: const float* (planes [B][2P][N][N]), NpStates or LnRows (Q = 1)
__global__ __launch_bounds__(kLnThreads, 1) void k_leafnet_np(In in, int B, const h16x8* __restrict__ wstem_a,
                                                              const float* __restrict__ sstem_a,
                                                              const float* __restrict__ bstem_a,
                                                              const h16x8* __restrict__ wt_a,
                                                              const float* __restrict__ st_a,
                                                              const float* __restrict__ bt_a,
                                                              const float* __restrict__ bounds_a, int nlayers,
                                                              LnHeads hd_a, float* __restrict__ xout) {
  // ROWS (bk_leafnet_x3_rows): the STATES form on state row tree[blockIdx.x] with the row's own
  // weight set, as in k_leafnet_x3; the *_a weight arguments are unused (null) then
  constexpr bool ROWS = std::is_same<In, LnRows>::value;
  static_assert(!ROWS || Q == 1, "k_leafnet_np: rows of one workgroup could belong to different nets");
  const h16x8* __restrict__ wstem = wstem_a;
  const float* __restrict__ sstem = sstem_a;
  const float* __restrict__ bstem = bstem_a;
  const h16x8* __restrict__ wt = wt_a;
  const float* __restrict__ st = st_a;
  const float* __restrict__ bt = bt_a;
  const float* __restrict__ bounds = bounds_a;
  LnHeads hd = hd_a;
  int row_tree = 0;
  if constexpr (ROWS) {
    // workgroup-uniform, before any barrier or LDS use
    int k;
    row_tree = ln_row_tree(in, blockIdx.x, k);
    if (row_tree < 0) return;
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
  using G = NpGeo<N, Q>;
  constexpr bool STATES = std::is_same<In, NpStates>::value || ROWS;
  constexpr int NN = G::NN, NPIX = G::NPIX, RS = G::RS, NG = G::NG, PL = G::PL, X0L = G::X0L;
  constexpr int PIX_IT = (NPIX + kLnThreads - 1) / kLnThreads;
  constexpr int QX = Q == 4 ? Q + 1 : Q;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  unsigned char* act = lds;             // 16 planes [hi q | lo q][GR x RS slots][16 B]
  unsigned char* sin = lds + 16 * PL;   // 2 planes: the stem input hi, lo
  float* red = reinterpret_cast<float*>(lds + G::kLdsBody);  // [3][Q][4 waves]: layer parity 0, 1, the observation
  f32x4* x0s = reinterpret_cast<f32x4*>(lds + 16 * PL);
  const int tid = threadIdx.x, l = tid & 63, n = l & 15, ks = l >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int oc = 16 * wave + 4 * ks;
  const int P = hd.P;
  const int b0 = ROWS ? row_tree : blockIdx.x * Q;  // the workgroup's boards b0 .. b0 + nb - 1 (ROWS: the row's tree)
  const int nb = ROWS ? 1 : (B - b0 < Q ? B - b0 : Q);  // a tail workgroup: boards nb.. are all-zero, never loaded or stored

  // the observation loads first (their latency under the halo zeroing below)
  float xin[STATES ? 1 : PIX_IT][kStemCinX3];
  constexpr int SW_IT = (Q * kNpRowStride + kLnThreads - 1) / kLnThreads;
  uint32_t sw[SW_IT];   // STATES: word i = tid + it * 256 of the workgroup's [Q][P kMaxN rows | to_move]
  bool slive[SW_IT];
  const int RW = P * kMaxN;  // row words per board
  if constexpr (STATES) {
#pragma unroll
    for (int it = 0; it < SW_IT; ++it) {
      const int i = tid + it * kLnThreads;
      const int q = Q == 1 ? 0 : i / (RW + 1), k = i - q * (RW + 1);
      // ROWS: a leaf, or the workgroup has returned
      slive[it] = i < Q * (RW + 1) && q < nb && (ROWS || !in.status || in.status[b0 + q] == 1);
      sw[it] = slive[it] ? in.states[(size_t)(b0 + q) * kStateWords + (k < RW ? k : kWToMove)] : 0u;
    }
  } else {
#pragma unroll
    for (int it = 0; it < PIX_IT; ++it) {
      const int p = tid + it * kLnThreads;
      const int q = Q == 1 ? 0 : p / NN;
      const bool ok = p < NPIX && q < nb;
      const float* __restrict__ ob = in + ((size_t)(b0 + q) * 2 * P) * NN + (p - q * NN);
#pragma unroll
      for (int c = 0; c < kStemCinX3; ++c) xin[it][c] = ok && c < 2 * P ? ob[c * NN] : 0.0f;
    }
  }
  // zero every slot that is no pixel, in all 18 planes (STATES: 17, no lo plane of the stem
  // input): the border and, Q = 4, the separators between the boards. The only slots read that
  // no layer writes.
  for (int s = tid; s < G::GR * RS; s += kLnThreads) {
    if (!G::is_pixel(s)) {
#pragma unroll
      for (int plane = 0; plane < (STATES ? 17 : 18); ++plane)
        *reinterpret_cast<u32x4*>(lds + plane * PL + s * 16) = u32x4{0u, 0u, 0u, 0u};
    }
  }

  // ab[g] = the lane's B-read base in group g (its slot + its k-group's plane block, less kBias,
  // as k_leafnet_x3); a spare column reads at the first pixel (its MFMA column is never written
  // out).
  constexpr int kBias = (RS + 1) * 16;
  int ab[NG];
  unsigned valid = 0;
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    const int sl = kNpPixMap<N, Q>.slot[16 * g + n];
    ab[g] = (sl >= 0 ? sl : RS + 1) * 16 + ks * 4 * PL - kBias;
    valid |= (sl >= 0 ? 1u : 0u) << g;
  }
  auto is_valid = [&](int g) { return NPIX % 16 == 0 || ((valid >> g) & 1u); };
  auto slot_b = [&](int g) { return ab[g] - ks * 4 * PL + kBias; };
  // the board of the lane's column in group g: a constant but in group 12 of Q = 4 (NpPixMap),
  // where it is n & 3. Per-board registers (scales, maxima) have QX entries: the Q boards, then
  // (Q = 4) the lane's own board of group 12, so that every index is a compile-time constant
  auto board_of = [&](int g) { return Q == 1 ? 0 : (g < 12 ? g / 3 : n & 3); };
  auto bidx = [&](int g) { return Q == 1 ? 0 : (g < 12 ? g / 3 : Q); };
  // the lane's cell in its board, from its slot in group g
  auto cell_of = [&](int g) {
    const int sl = slot_b(g) / 16;
    int rr = sl / RS - 1, cc = sl % RS - 1;
    if constexpr (Q == 4) {
      rr -= rr > N ? N + 1 : 0;
      cc -= cc > N ? N + 1 : 0;
    }
    return rr * N + cc;
  };

  static_assert(18 % (kLnWpf + 1) == 0, "kLnWpf: the ring must divide the 18 chunks of a layer");
  constexpr int kLayerBlocks = 18 * 4 * 2;
  const __amdgpu_buffer_rsrc_t wrs = ln_rsrc(wt, (unsigned)nlayers * kLayerBlocks * 1024u);
  auto wload = [&](int layer, int c, int p) {
    return __builtin_bit_cast(h16x8, __builtin_amdgcn_raw_buffer_load_b128(
                                         wrs, l * 16, ((layer * kLayerBlocks + c * 8 + wave * 2 + p) * 64) * 16, 0));
  };
  h16x8 wq[kLnWpf + 1][2];
#pragma unroll
  for (int c = 0; c < kLnWpf; ++c) {
    wq[c][0] = wload(0, c, 0);
    wq[c][1] = wload(0, c, 1);
  }
  h16x8 wsa[3][2];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    wsa[j][0] = wstem[((j * 4 + wave) * 2) * 64 + l];
    wsa[j][1] = wstem[((j * 4 + wave) * 2 + 1) * 64 + l];
  }
  const f32x4 s_stem = *reinterpret_cast<const f32x4*>(sstem + oc), b_stem = *reinterpret_cast<const f32x4*>(bstem + oc);

  // per-board maxima: every lane's m[q] -> red[(slot * Q + q) * 4 + wave] before a barrier, the
  // board's maximum after it (a maximum of non-negative floats: exact in any order)
  auto post_max = [&](const float (&m)[Q], int slot) {
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const float w = wave_max_f(m[q]);
      if (l == 0) red[(slot * Q + q) * 4 + wave] = w;
    }
  };
  auto board_max = [&](int slot, int q) {
    const float* r = red + (slot * Q + q) * 4;
    return fmaxf(fmaxf(r[0], r[1]), fmaxf(r[2], r[3]));
  };
  auto board_maxima = [&](int slot, float (&m)[QX]) {
#pragma unroll
    for (int q = 0; q < Q; ++q) m[q] = board_max(slot, q);
    if constexpr (QX > Q) m[Q] = board_max(slot, n & 3);
  };

  // ---- stem input: each board's observation scaled by the board's own maximum, split
  float max_obs[QX];
  int ex[QX];
  if constexpr (STATES) {
    // the boards' row words (bits past the board dropped) and to_move staged in the unused lo
    // plane's space; a board's maximum is 1 iff any plane has a cell set: a row bit, or a to_move
    // that names one of the P mover planes
    uint32_t* rows = reinterpret_cast<uint32_t*>(sin + PL);
    float any[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) any[q] = 0.0f;
#pragma unroll
    for (int it = 0; it < SW_IT; ++it) {
      const int i = tid + it * kLnThreads;
      const int q = Q == 1 ? 0 : i / (RW + 1), k = i - q * (RW + 1);
      if (i < Q * (RW + 1)) {
        bool a;
        if (k < RW) {
          const uint32_t bits = k % kMaxN < N ? sw[it] & ((1u << N) - 1u) : 0u;
          rows[q * kNpRowStride + k] = bits;
          a = bits != 0u;
        } else {
          const uint32_t tm = slive[it] ? sw[it] : ~0u;  // no mover plane of a board that is not a leaf
          rows[q * kNpRowStride + kNpRowStride - 1] = tm;
          a = tm < (uint32_t)P;
        }
#pragma unroll
        for (int qq = 0; qq < Q; ++qq) any[qq] = a && q == qq ? 1.0f : any[qq];
      }
    }
    post_max(any, 2);
    __syncthreads();  // the zeroing and the rows before the writes
    board_maxima(2, max_obs);
#pragma unroll
    for (int q = 0; q < QX; ++q) ex[q] = scale_exp(max_obs[q]);
#pragma unroll
    for (int it = 0; it < PIX_IT; ++it) {
      const int p = tid + it * kLnThreads;
      if (p < NPIX) {
        const int q = Q == 1 ? 0 : p / NN, cell = p - q * NN, r = cell / N, c = cell % N;
        // a set cell's hi half: f16(2^ex), what split2 gives the planar form's 1.0f * 2^ex
        const unsigned one = __builtin_bit_cast(unsigned short, (_Float16)ldexpf(1.0f, scale_exp(board_max(2, q))));
        const uint32_t* rw = rows + q * kNpRowStride;
        const uint32_t tm = rw[kNpRowStride - 1];
        unsigned val[kStemCinX3];  // channels 0..P-1 the boards, P..2P-1 the mover planes, then zeros
#pragma unroll
        for (int ch = 0; ch < kStemCinX3; ++ch) {
          const unsigned bit = ch < kMaxP ? (rw[(ch < P ? ch : 0) * kMaxN + r] >> c) & 1u : 0u;
          val[ch] = ch < P ? bit : (ch < 2 * P && tm == (uint32_t)(ch - P) ? 1u : 0u);
        }
        // channels 2j (low 16 bits), 2j + 1 (high) per word, as split2 packs them
        const u32x4 hi{(val[0] | (val[1] << 16)) * one, (val[2] | (val[3] << 16)) * one,
                       (val[4] | (val[5] << 16)) * one, (val[6] | (val[7] << 16)) * one};
        *reinterpret_cast<u32x4*>(sin + G::slot_of(p) * 16) = hi;
      }
    }
  } else {
    float m[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) m[q] = 0.0f;
#pragma unroll
    for (int it = 0; it < PIX_IT; ++it) {
      const int p = tid + it * kLnThreads;
      const int q = Q == 1 ? 0 : p / NN;
      float mm = 0.0f;
#pragma unroll
      for (int c = 0; c < kStemCinX3; ++c) mm = fmaxf(mm, fabsf(xin[it][c]));
#pragma unroll
      for (int qq = 0; qq < Q; ++qq) m[qq] = q == qq ? fmaxf(m[qq], mm) : m[qq];
    }
    post_max(m, 2);
    __syncthreads();  // also orders the zeroing before the writes
    board_maxima(2, max_obs);
#pragma unroll
    for (int q = 0; q < QX; ++q) ex[q] = scale_exp(max_obs[q]);
#pragma unroll
    for (int it = 0; it < PIX_IT; ++it) {
      const int p = tid + it * kLnThreads;
      if (p < NPIX) {
        const int e = scale_exp(board_max(2, Q == 1 ? 0 : p / NN));
        unsigned h[4], o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) split2(ldexpf(xin[it][2 * j], e), ldexpf(xin[it][2 * j + 1], e), h[j], o[j]);
        const u32x4 hi{h[0], h[1], h[2], h[3]}, lo{o[0], o[1], o[2], o[3]};
        unsigned char* dst = sin + G::slot_of(p) * 16;
        *reinterpret_cast<u32x4*>(dst) = hi;
        *reinterpret_cast<u32x4*>(dst + PL) = lo;
      }
    }
  }
  __syncthreads();

  // ---- stem conv: 3 chunks; lane k-group ks of chunk j is tap 4j + ks (taps > 8 carry zero weights)
  f32x4 acc[NG];
  h16x8 rb[kLnSlots][2];
  {
    auto toff = [&](int j) {
      const int t = 4 * j + ks < 9 ? 4 * j + ks : 8;
      return ((t / 3 - 1) * RS + (t % 3 - 1)) * 16 + kBias - ks * 4 * PL;  // from ab: the stem grid has 2 planes
    };
    if constexpr (STATES) {  // no lo plane: two products per chunk
      ln_prime_hi<NG>(rb, sin, ab, toff(0));
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        if (j == 0)
          ln_chunk_hi<NG, true>(acc, wsa[0][0], wsa[0][1], sin, ab, toff(0), toff(1), rb);
        else
          ln_chunk_hi<NG, false>(acc, wsa[j][0], wsa[j][1], sin, ab, toff(j), toff(j < 2 ? j + 1 : j), rb);
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

  // Epilogue of a conv, as k_leafnet_x3's: y = acc * s + bias (+ x0) (ReLU) with s = the inverse
  // weight scale x 2^(k - ex), bias x 2^k, k = the output scale (OUT) or 0, all powers of two
  // taken per column from the column's board; mx[q] = board q's largest |y|, unscaled. OUT: y is
  // split and stored into the grid in place (after the caller's barrier); else y stays in acc.
  auto epilogue = [&](f32x4 sv, f32x4 bv, bool relu, bool residual, const f32x4 (&x0)[NG], bool out,
                      const int (&ex_out)[QX], float (&mxo)[Q]) {
    const int o = 2 * wave + (ks >> 1);
    unsigned char* wbase = act + ((o & 3) * 4 + (o >> 2) * 2) * PL + (ks & 1) * 8;
    int kk[QX], dd[QX];
    float mx[Q];
#pragma unroll
    for (int q = 0; q < QX; ++q) {
      kk[q] = out ? ex_out[q] : 0;
      dd[q] = kk[q] - ex[q];
    }
#pragma unroll
    for (int q = 0; q < Q; ++q) mx[q] = 0.0f;
    const int floor = relu ? 0 : (int)0x80000000u;
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      const int q = board_of(g);
      const int k = kk[bidx(g)], d = dd[bidx(g)];
      const f32x2 s01{ldexpf(sv.x, d), ldexpf(sv.y, d)}, s23{ldexpf(sv.z, d), ldexpf(sv.w, d)};
      const f32x2 b01{ldexpf(bv.x, k), ldexpf(bv.y, k)}, b23{ldexpf(bv.z, k), ldexpf(bv.w, k)};
      f32x2 y01 = pk_fma(f32x2{acc[g][0], acc[g][1]}, s01, b01);
      f32x2 y23 = pk_fma(f32x2{acc[g][2], acc[g][3]}, s23, b23);
      if (residual) {  // only without OUT (the last conv): x0 is unscaled
        y01 = pk_add(y01, f32x2{x0[g][0], x0[g][1]});
        y23 = pk_add(y23, f32x2{x0[g][2], x0[g][3]});
      }
      y01 = f32x2{max_bits(y01.x, floor), max_bits(y01.y, floor)};
      y23 = f32x2{max_bits(y23.x, floor), max_bits(y23.y, floor)};
      if (is_valid(g)) {
        if constexpr (Q == 1) {
          mx[0] = max3_abs(max3_abs(mx[0], y01.x, y01.y), y23.x, y23.y);
        } else {
          const float m = max3_abs(max3_abs(0.0f, y01.x, y01.y), y23.x, y23.y);
#pragma unroll
          for (int qq = 0; qq < Q; ++qq) mx[qq] = q == qq ? max3_abs(mx[qq], m, m) : mx[qq];
        }
      }
      if (out) {
        unsigned h0, h1, l0, l1;
        split2(y01.x, y01.y, h0, l0);
        split2(y23.x, y23.y, h1, l1);
        if (is_valid(g)) {
          *reinterpret_cast<u32x2*>(wbase + slot_b(g)) = u32x2{h0, h1};
          *reinterpret_cast<u32x2*>(wbase + slot_b(g) + PL) = u32x2{l0, l1};
        }
      } else {
        acc[g] = f32x4{y01.x, y01.y, y23.x, y23.y};
      }
    }
#pragma unroll
    for (int q = 0; q < Q; ++q) mxo[q] = ldexpf(mx[q], -kk[q]);
  };

  f32x4 x0[NG];
  float max_in[QX];
  {
    int ex_out[QX];
    float mx[Q];
#pragma unroll
    for (int q = 0; q < QX; ++q) ex_out[q] = scale_exp(bounds[0] * max_obs[q] + bounds[1]);
#pragma unroll
    for (int g = 0; g < NG; ++g) x0[g] = f32x4{0.f, 0.f, 0.f, 0.f};
    // the stem output itself is kept (unscaled) for the tower's final residual
    epilogue(s_stem, b_stem, true, false, x0, false, ex_out, mx);
#pragma unroll
    for (int g = 0; g < NG; ++g) x0[g] = acc[g];
    post_max(mx, 0);
    __syncthreads();  // every wave is done with the stem's input planes (the x0 stash reuses them)
    {
      const int o = 2 * wave + (ks >> 1);
      unsigned char* base = act + ((o & 3) * 4 + (o >> 2) * 2) * PL + (ks & 1) * 8;
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        const float up = ldexpf(1.0f, ex_out[bidx(g)]);
        unsigned h0, h1, l0, l1;
        split2(x0[g][0] * up, x0[g][1] * up, h0, l0);
        split2(x0[g][2] * up, x0[g][3] * up, h1, l1);
        if (is_valid(g)) {
          *reinterpret_cast<u32x2*>(base + slot_b(g)) = u32x2{h0, h1};
          *reinterpret_cast<u32x2*>(base + slot_b(g) + PL) = u32x2{l0, l1};
        }
      }
    }
    // x0 waits out the tower in AGPRs (read once, by the last conv), 20x20: its first groups in LDS
#pragma unroll
    for (int g = X0L; g < NG; ++g) asm volatile("" : "+a"(x0[g]));
#pragma unroll
    for (int g = 0; g < X0L; ++g) {
      x0s[g * kLnThreads + tid] = x0[g];
      x0[g] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    __syncthreads();
    board_maxima(0, max_in);
#pragma unroll
    for (int q = 0; q < QX; ++q) ex[q] = ex_out[q];
  }

  // ---- residual tower: nlayers convs 64 -> 64; ReLU after each block's first conv; the last
  // adds x0 and takes the ReLU
  for (int layer = 0; layer < nlayers; ++layer) {
    const bool more = layer + 1 < nlayers;
    const f32x4 sv = *reinterpret_cast<const f32x4*>(st + layer * 64 + oc);
    const f32x4 bv = *reinterpret_cast<const f32x4*>(bt + layer * 64 + oc);
    const float bnd_a = bounds[2 * (layer + 1)], bnd_b = bounds[2 * (layer + 1) + 1];
    auto coff_of = [&](int c) {
      const int t = c >> 1;
      return 2 * (c & 1) * PL + ((t / 3 - 1) * RS + (t % 3 - 1)) * 16 + kBias;
    };
    ln_prime<NG, PL>(rb, act, ab, coff_of(0));
#pragma unroll
    for (int c = 0; c < 18; ++c) {
      const int cn = c + kLnWpf, sn = cn % (kLnWpf + 1);
      if (cn < 18) {
        wq[sn][0] = wload(layer, cn, 0);
        wq[sn][1] = wload(layer, cn, 1);
      } else {  // the next layer's first chunks (the last layer reloads its own, never used)
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
    // the last chunk's read-ahead (ln_chunk_il: untracked) lands before its registers are reused
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    ln_mfma_drain(acc);
    if (more) {
      int ex_out[QX];
      float mx[Q];
#pragma unroll
      for (int q = 0; q < QX; ++q) ex_out[q] = scale_exp(bnd_a * max_in[q] + bnd_b);
      __syncthreads();  // every wave has finished reading the grid: the outputs go in place as made
      epilogue(sv, bv, !(layer & 1), false, x0, true, ex_out, mx);
      post_max(mx, (layer + 1) & 1);
      __syncthreads();
      board_maxima((layer + 1) & 1, max_in);
#pragma unroll
      for (int q = 0; q < QX; ++q) ex[q] = ex_out[q];
    } else {
      int none[QX];
      float mx[Q];
#pragma unroll
      for (int q = 0; q < QX; ++q) none[q] = 0;
#pragma unroll
      for (int g = 0; g < X0L; ++g) x0[g] = x0s[g * kLnThreads + tid];
      epilogue(sv, bv, true, true, x0, false, none, mx);
    }
  }

  // ---- outputs: the tower output (optional) and the heads
  if (xout) {
#pragma unroll
    for (int g = 0; g < NG; ++g)
      if (is_valid(g) && board_of(g) < nb)
        *reinterpret_cast<f32x4*>(xout + ((size_t)(b0 + board_of(g)) * NN + cell_of(g)) * 64 + oc) = acc[g];
  }
  __syncthreads();  // every wave is done with the activation grid: the heads' scratch reuses it
  float* hp = reinterpret_cast<float*>(act);  // [NPIX][4 waves][3]
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
        // the sum over the 4 k-groups: a + a(lane ^ 16), then + (lane ^ 32) (VALU swaps)
        const float a = y.x * (*w[k]).x + y.y * (*w[k]).y + y.z * (*w[k]).z + y.w * (*w[k]).w;
        const auto s16 = __builtin_amdgcn_permlane16_swap(__float_as_uint(a), __float_as_uint(a), false, false);
        const float a16 = __uint_as_float(s16[0]) + __uint_as_float(s16[1]);
        const auto s32 = __builtin_amdgcn_permlane32_swap(__float_as_uint(a16), __float_as_uint(a16), false, false);
        d[k] = __uint_as_float(s32[0]) + __uint_as_float(s32[1]);
      }
      if (ks == 0 && is_valid(g)) {
        float* dst = hp + ((board_of(g) * NN + cell_of(g)) * 4 + wave) * 3;
        dst[0] = d[0];
        dst[1] = d[1];
        dst[2] = d[2];
      }
    }
  }
  __syncthreads();
  // pf = relu(policy 1x1 conv + bp) (channel-major), vfeat = relu(value 1x1 conv + bv): the four
  // waves' partial sums added in wave order
  float* vfeat = hp + NPIX * 12;  // [Q][NN]
  float* part = vfeat + NPIX;     // [Q][4 waves][64]
  const float bp0 = hd.bp[0], bp1 = hd.bp[1], bv0 = hd.bv[0];
  for (int i = tid; i < NPIX; i += kLnThreads) {
    const int q = Q == 1 ? 0 : i / NN, cell = i - q * NN;
    const float* h = hp + i * 12;
    const float p0 = ((h[0] + h[3]) + h[6]) + h[9], p1 = ((h[1] + h[4]) + h[7]) + h[10],
                pv = ((h[2] + h[5]) + h[8]) + h[11];
    if (q < nb) {
      hd.pf[(size_t)(b0 + q) * 2 * NN + cell] = fmaxf(p0 + bp0, 0.0f);
      hd.pf[(size_t)(b0 + q) * 2 * NN + NN + cell] = fmaxf(p1 + bp1, 0.0f);
    }
    vfeat[i] = fmaxf(pv + bv0, 0.0f);
  }
  __syncthreads();
  {
    // v = tanh(W2 relu(W1 vfeat + b1) + b2). The summation order of W1 vfeat, the same for every
    // board in either workgroup form: wave w takes the inputs k0 + j, k0 = CH w, j = 0..CH-1,
    // CH = ceil(NN / 4) (inputs past NN count as 0 x 0); lane l's row l. Over j ascending, in
    // blocks of 10: a0 += the even j, a1 += the odd j; the last CH % 10 all into a0; the wave's
    // part = a0 + a1; h = relu(((part0 + part1) + (part2 + part3)) + b1).
    constexpr int CH = (NN + 3) / 4;
    const int k0 = CH * wave;
    float w[CH];
#pragma unroll
    for (int j = 0; j < CH; ++j) w[j] = k0 + j < NN ? hd.w1t[(size_t)(k0 + j) * 64 + l] : 0.0f;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const float* vf = vfeat + q * NN;
      float a0 = 0.f, a1 = 0.f;
      int j = 0;
#pragma unroll
      for (; j + 10 <= CH; j += 10) {
#pragma unroll
        for (int u = 0; u < 10; u += 2) {
          a0 += w[j + u] * (k0 + j + u < NN ? vf[k0 + j + u] : 0.0f);
          a1 += w[j + u + 1] * (k0 + j + u + 1 < NN ? vf[k0 + j + u + 1] : 0.0f);
        }
      }
#pragma unroll
      for (; j < CH; ++j) a0 += w[j] * (k0 + j < NN ? vf[k0 + j] : 0.0f);
      part[(q * 4 + wave) * 64 + l] = a0 + a1;
    }
  }
  __syncthreads();
  if (wave < Q && wave < nb) {  // wave q: board q's value row
    const float* pt = part + wave * 256;
    float w2[kMaxP], b2[kMaxP];
#pragma unroll
    for (int q = 0; q < kMaxP; ++q) {
      w2[q] = q < P ? hd.w2[q * 64 + l] : 0.0f;
      b2[q] = q < P ? hd.b2[q] : 0.0f;
    }
    const float h = fmaxf(((pt[l] + pt[64 + l]) + (pt[128 + l] + pt[192 + l])) + hd.b1[l], 0.0f);
#pragma unroll
    for (int q = 0; q < kMaxP; ++q) {
      if (q < P) {
        const float sum = wave_sum_f(w2[q] * h);
        if (l == 0) hd.v[(size_t)(b0 + wave) * P + q] = tanhf(sum + b2[q]);
      }
    }
  }
}

static_assert(NpGeo<20, 1>::kLds <= 160 * 1024, "k_leafnet_np<20>: LDS");

// the launch of one instantiation: B boards with the weight set w and the heads h
template <int N, int Q, typename In>
int np_launch(In in, int B, const LnNet& w, int nlayers, const LnHeads& h, float* out, hipStream_t s) {
  const void* fn = (const void*)k_leafnet_np<N, Q, In>;
  constexpr int kLds = NpGeo<N, Q>::kLds;
  if (set_max_dynamic_lds(&fn, 1, kLds) != BK_OK) return BK_EHIP;
  hipLaunchKernelGGL((k_leafnet_np<N, Q, In>), dim3((B + Q - 1) / Q), dim3(kLnThreads), kLds, s, in, B, w.wstem,
                     w.sstem, w.bstem, w.wt, w.st, w.bt, w.bounds, nlayers, h, out);
  return launch_check("k_leafnet_np");
}

// Boards per workgroup when the caller leaves it open (7x7 only). Model: rounds of workgroups x
// pixel groups per workgroup, ceil(B / (Q CUs)) NG(Q) with NG(1) = 5 and NG(4) = 15. Measured
// (profiles/leafnet_np_bench.json) it orders every timed B: one board per workgroup
// wins at 64, 256 and 512, four at 1024 and 4096; at the tie of 768 four boards are 6% faster
// with 5 blocks and 2% slower with 2, so a tie goes to four.
int np_boards(int N, int B, int boards_per_wg) {
  if (boards_per_wg) return boards_per_wg;
  if (N != 7) return 1;
  static const int cus = [] {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
      n = 256;
    return n;
  }();
  const int r1 = (B + cus - 1) / cus, r4 = (B + 4 * cus - 1) / (4 * cus);
  return 5 * r1 >= 15 * r4 ? 4 : 1;
}

// One launch of k_leafnet_np on B boards, Q per workgroup: the weight set w, rows t0.. of a's
// outputs and of the whole-batch tower output `out` (may be null). The rows form passes an empty
// w, t0 = 0 and B = R workgroups of one board each (the kernel takes its board from the row table).
template <typename In>  // const float* (the planes of row t0), NpStates (at row t0) or LnRows
int np_run(In in, int B, int Q, const bk_leafnet_args& a, const LnNet& w, int t0, float* out, void* stream) {
  const LnHeads h = ln_heads_of(a, w, t0);
  float* xout = out ? out + (size_t)t0 * a.N * a.N * 64 : nullptr;
  hipStream_t s = (hipStream_t)stream;
  if constexpr (!std::is_same<In, LnRows>::value)
    if (a.N == 7 && Q == 4) return np_launch<7, 4, In>(in, B, w, a.nlayers, h, xout, s);
  if (a.N == 7) return np_launch<7, 1, In>(in, B, w, a.nlayers, h, xout, s);
  if (a.N == 14) return np_launch<14, 1, In>(in, B, w, a.nlayers, h, xout, s);
  return np_launch<20, 1, In>(in, B, w, a.nlayers, h, xout, s);
}

}  // namespace

int leafnet_np_run(const bk_leafnet_args* nets, int nnets, const bk_arena_rows* rows, int sim, int t0, int n,
                   float* out, void* stream) {
  const bk_leafnet_args& a = nets[0];
  if (rows) return np_run(ln_rows_of(nets, nnets, rows, sim), rows->R, 1, a, LnNet{}, 0, nullptr, stream);
  const int Q = np_boards(a.N, n, a.np - 1);
  const LnNet w = ln_net_of(a);
  if (a.obs) return np_run(a.obs + (size_t)t0 * 2 * a.P * a.N * a.N, n, Q, a, w, t0, out, stream);
  return np_run(ln_states_of<NpStates>(a, t0), n, Q, a, w, t0, out, stream);
}
}  // namespace bk

using namespace bk;

extern "C" {

int bk_leafnet_x3_np_supported(int N, int P) { return (N == 7 || N == 14 || N == 20) && P >= 2 && P <= kMaxP; }

// Wrappers over bk_leafnet_x3_run (leafnet.hip): boards_per_wg folded into the struct's np.
int bk_leafnet_x3_np(const float* obs, int B, int N, int cin, const void* wstem, const float* sstem,
                     const float* bstem, int nlayers, const void* wtower, const float* stower, const float* btower,
                     const float* bounds, const float* wp, const float* bp, const float* wv, const float* bv,
                     const float* w1t, const float* b1, const float* w2, const float* b2, int P, float* pf,
                     float* vout, float* out, int boards_per_wg, void* stream) {
  BK_REQUIRE(cin == 2 * P, "bk_leafnet_x3_np: the observation has 2 P planes");
  BK_REQUIRE(boards_per_wg == 0 || boards_per_wg == 1 || (boards_per_wg == 4 && N == 7),
             "bk_leafnet_x3_np: boards_per_wg must be 0, 1 or (N = 7 only) 4");
  const bk_leafnet_args a{obs, nullptr, nullptr, N,  P,  nlayers, wstem, sstem, bstem, wtower, stower, btower,
                          bounds, wp,   bp,      wv, bv, w1t,     b1,    w2,    b2,    pf,     vout,   boards_per_wg + 1};
  return bk_leafnet_x3_run(&a, 0, B, out, stream);
}

int bk_leafnet_x3_np_states(const void* states, const int32_t* status, int B, int N, int P, const void* wstem,
                            const float* sstem, const float* bstem, int nlayers, const void* wtower,
                            const float* stower, const float* btower, const float* bounds, const float* wp,
                            const float* bp, const float* wv, const float* bv, const float* w1t, const float* b1,
                            const float* w2, const float* b2, float* pf, float* vout, float* out, int boards_per_wg,
                            void* stream) {
  BK_REQUIRE(boards_per_wg == 0 || boards_per_wg == 1 || (boards_per_wg == 4 && N == 7),
             "bk_leafnet_x3_np_states: boards_per_wg must be 0, 1 or (N = 7 only) 4");
  const bk_leafnet_args a{nullptr, states, status, N,  P,  nlayers, wstem, sstem, bstem, wtower, stower, btower,
                          bounds,  wp,     bp,     wv, bv, w1t,     b1,    w2,    b2,    pf,     vout,   boards_per_wg + 1};
  return bk_leafnet_x3_run(&a, 0, B, out, stream);
}

}  // extern "C"

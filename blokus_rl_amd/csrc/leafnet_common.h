// leafnet_common.h — pieces shared by the leaf-net kernels on split-f16 MFMA products
// (leafnet.hip: k_leafnet_x3, direct convolutions): the operand split, power-of-two scaling, the
// stem's pixel map and direct K-chunk loop, the MFMA drain.
#pragma once
#include "../../include/blokus_engine.h"
#include "ctx.h"

#include <type_traits>
#include <utility>

namespace bk {
// bk_leafnet_x3_run / bk_leafnet_x3_rows on the np kernels (leafnet_np.hip), the operands validated
// by the caller (leafnet.hip ln_check). rows null: boards [t0, t0 + n) of nets[0], n > 0, with
// out as bk_leafnet_x3_run's. Else the rows of the table `nets` at `sim`: one board per workgroup
// whatever np's boards_per_wg says (the rows of a four-board workgroup could belong to different
// nets); a board's outputs do not depend on the form, so they are bitwise those of the range.
int leafnet_np_run(const bk_leafnet_args* nets, int nnets, const bk_arena_rows* rows, int sim, int t0, int n,
                   float* out, void* stream);

namespace {

using h16x8 = _Float16 __attribute__((ext_vector_type(8)));
using h16x2 = _Float16 __attribute__((ext_vector_type(2)));
using f32x4 = float __attribute__((ext_vector_type(4)));
using f32x2 = float __attribute__((ext_vector_type(2)));
using u32x4 = unsigned __attribute__((ext_vector_type(4)));
using u32x2 = unsigned __attribute__((ext_vector_type(2)));

#ifndef BK_LN_DUMMY
#define BK_LN_DUMMY 0  // timing diagnostic only: dummy VALU ops after each MFMA triple (ln_chunk;
                       // profiles/r06_leafnet_valu_shadow.json: ~5.5 cycles each, not hidden)
#endif
#ifndef BK_LN_STAMP
#define BK_LN_STAMP 0  // timing diagnostics only: per-wave s_memtime stamps (bk_ln_stamps)
#endif
#if BK_LN_STAMP
constexpr int kLnStamps = 48;
__device__ unsigned long long g_ln_stamps[256 * 4 * kLnStamps];
#define LNSTAMP(i, v)                                                                                          \
  do {                                                                                                         \
    if (l == 0 && blockIdx.x < 256) g_ln_stamps[(blockIdx.x * 4 + wave) * kLnStamps + (i)] = (v);              \
  } while (0)
#else
#define LNSTAMP(i, v) \
  do {                \
  } while (0)
#endif

constexpr int kLnThreads = 256;
constexpr int kStemCinX3 = 8;
constexpr int kBlock = 64 * 8;     // f16 per (chunk, wave, part) block of packed weights: 64 lanes x 8

__host__ __device__ constexpr int ln_chunks(int cin) { return cin == 64 ? 18 : 3; }

// B-fragment pipeline: the grid reads of a group are issued kLnPf groups ahead of its MFMAs, in a
// ring of kLnSlots register slots that runs on across chunk boundaries (the last kLnPf groups of
// a chunk load the first kLnPf of the next), so the LDS latency is never exposed at a chunk start.
// The slot of group g is g % kLnSlots in every chunk, which needs NG % kLnSlots == 0: the board's
// groups are padded with spare ones (all columns spare: halo reads, no writes) up to a multiple.
// (ln_chunk_il_act, whose chunks differ in length, takes the slot from the position in the layer's
// sequence of active (chunk, group) pairs instead.)
#ifndef BK_LN_VACC
#define BK_LN_VACC 0  // the MFMA accumulators in VGPRs (1: leafnet.hip, and leafnet_w3.hip, whose AGPRs hold U) or AGPRs (0)
#endif
#if BK_LN_VACC
#define BK_ACC_W "=&v"
#define BK_ACC_RW "+v"
#else
#define BK_ACC_W "=&a"
#define BK_ACC_RW "+a"
#endif
// read-ahead: 2 groups of B fragments (3, 4: no gain, also with ln_chunk_il), 1 chunk of weights (2: no gain)
constexpr int kLnPf = 2, kLnSlots = 5, kLnWpf = 1;
static_assert(kLnPf >= 1 && kLnPf < kLnSlots, "kLnPf");
__host__ __device__ constexpr int ln_groups(int N) { return ((N * N + 15) / 16 + kLnSlots - 1) / kLnSlots * kLnSlots; }

// The layer input in LDS: 16 planes, each a zero-haloed grid of (N+2) rows x ln_row(N) slots of
// 16 B (8 f16). Channel octet o (channels 8o..8o+7) has its hi halves in plane 4 (o % 4) + 2 (o / 4)
// and its lo halves in the next plane: the octets a lane's k-group ks reads (ks and 4 + ks) sit
// in its own block of 4 planes, so one base register per group reaches every chunk's tap and
// half with an immediate offset (< 3 planes + 2 rows). A plane
// is a multiple of 256 B (the LDS bank period), so the 16-B chunk of every plane of a slot sits in
// the same 4 banks, and the lanes of one ds_read_b128 lane group (16 distinct pixels of a group,
// k-groups ks and ks^1) are conflict-free when their slots differ mod 16 (LnPixMap). The stem's
// input (8 channels) takes two more planes (hi, lo).
__host__ __device__ constexpr int ln_row(int N) { return N == 14 ? 18 : N + 2; }  // slot classes mod 16 balanced
__host__ __device__ constexpr int ln_plane(int N) { return ((N + 2) * ln_row(N) * 16 + 255) / 256 * 256; }
// The stem output's groups that wait out the tower in LDS instead of registers (k_leafnet_x3<20>:
// the register file holds the other 18 groups; all 25 would spill 26 registers to scratch), in the
// stem planes' region (dead after the stem) and above it: [group][256 threads] x 16 B
__host__ __device__ constexpr int ln_x0_lds_groups(int N) { return N == 20 ? 7 : 0; }
// LDS bytes of k_leafnet_x3<N>: 16 activation planes, then the 2 stem planes or the x0 stash
// (whichever is larger), then the wave maxima (2 x 4 + 4 floats) and the waves' binary-board
// flags (4 floats, k_leafnet_x3's FAST planes form)
__host__ __device__ constexpr int ln_lds_body(int N) {
  return 16 * ln_plane(N) + (2 * ln_plane(N) > ln_x0_lds_groups(N) * 256 * 16 ? 2 * ln_plane(N)
                                                                                 : ln_x0_lds_groups(N) * 256 * 16);
}
__host__ __device__ constexpr int ln_lds_bytes(int N) { return ln_lds_body(N) + 64; }

// The board's pixels in MFMA columns: slot (g, n) of pixel group g, column n. Any bijection works
// (reads and writes use the same map); this one gives each group 16 pixels whose grid slots are
// distinct mod 16 where the slot classes allow (one pixel per class, leftovers fill the gaps),
// so the B-fragment reads are bank-conflict-free. Entries: grid slot (row + 1) * ln_row + col + 1,
// or -1 for a spare column (N*N not a multiple of 16).
template <int N>
struct LnPixMap {
  static constexpr int NN = N * N, NG = ln_groups(N), RS = ln_row(N);
  int slot[NG * 16];
  constexpr LnPixMap() : slot() {
    bool used[NN] = {};
    for (int i = 0; i < NG * 16; ++i) slot[i] = -1;
    for (int g = 0; g < NG; ++g)
      for (int r = 0; r < 16; ++r)
        for (int p = 0; p < NN; ++p) {
          const int sl = (p / N + 1) * RS + p % N + 1;
          if (!used[p] && sl % 16 == r) {
            used[p] = true;
            slot[g * 16 + r] = sl;
            break;
          }
        }
    int p = 0;
    for (int i = 0; i < NG * 16; ++i) {
      if (slot[i] >= 0) continue;
      while (p < NN && used[p]) ++p;
      if (p == NN) break;
      used[p] = true;
      slot[i] = (p / N + 1) * RS + p % N + 1;
    }
  }
};
template <int N>
__device__ constexpr LnPixMap<N> kLnPixMap{};

// The edge-aware map of the 20x20 board (k_leafnet_x3<20, In, true>). Its last four groups each
// hold 16 pixels of one board edge: row 0, row N-1 (columns 2..17), column 0, column N-1 (rows
// 2..17). For the three taps that look outward over its edge such a group's whole B fragment is
// halo, i.e. zero, and its MFMAs add only a*0 products: LnEdgeSched leaves them out. The other
// 336 pixels fill groups 0..NG-5 by LnPixMap's greedy rule. The two row groups hit every slot
// class mod 16 once; the two column groups (slots 22 apart: 6 mod 16) hit 8 classes twice, a
// 2-way conflict on 2 of 25 groups that no lane order avoids (each ds_read_b128 lane group holds
// all 16 columns of a group: leafnet.hip's plane blocks of the two k-groups share their banks).
template <int N>
struct LnEdgePixMap {
  static constexpr int NN = N * N, NG = ln_groups(N), RS = ln_row(N), G0 = NG - 4;
  static_assert(N == 20 && NG * 16 == NN, "LnEdgePixMap: the 20x20 board (no spare columns)");
  // pixel i of edge group e (0 top, 1 bottom, 2 left, 3 right)
  static constexpr int edge_pixel(int e, int i) {
    return e == 0 ? 2 + i : e == 1 ? (N - 1) * N + 2 + i : e == 2 ? (2 + i) * N : (2 + i) * N + N - 1;
  }
  int slot[NG * 16];
  constexpr LnEdgePixMap() : slot() {
    bool used[NN] = {};
    for (int i = 0; i < NG * 16; ++i) slot[i] = -1;
    for (int e = 0; e < 4; ++e)
      for (int i = 0; i < 16; ++i) {
        const int p = edge_pixel(e, i);
        used[p] = true;
        slot[(G0 + e) * 16 + i] = (p / N + 1) * RS + p % N + 1;
      }
    for (int g = 0; g < G0; ++g)
      for (int r = 0; r < 16; ++r)
        for (int p = 0; p < NN; ++p) {
          const int sl = (p / N + 1) * RS + p % N + 1;
          if (!used[p] && sl % 16 == r) {
            used[p] = true;
            slot[g * 16 + r] = sl;
            break;
          }
        }
    int p = 0;
    for (int i = 0; i < G0 * 16; ++i) {
      if (slot[i] >= 0) continue;
      while (p < NN && used[p]) ++p;
      if (p == NN) break;
      used[p] = true;
      slot[i] = (p / N + 1) * RS + p % N + 1;
    }
  }
};
template <int N>
__device__ constexpr LnEdgePixMap<N> kLnEdgePixMap{};

// The tower's (group, chunk) schedule on LnEdgePixMap: chunk c of a 64 -> 64 conv is tap c / 2 =
// (dy + 1) * 3 + (dx + 1); the top group skips dy < 0 (chunks 0-5), the bottom group dy > 0
// (12-17), the left group dx < 0 (0, 1, 6, 7, 12, 13), the right group dx > 0 (4, 5, 10, 11, 16,
// 17): 24 of a conv's 450 (group, chunk) pairs. active(c): the groups chunk c runs, as a bit mask;
// first(c): those it runs first (the INIT form); pos0(c): the active pairs before chunk c.
template <int N>
struct LnEdgeSched {
  static constexpr int NG = ln_groups(N), G0 = NG - 4, NC = ln_chunks(64);
  static constexpr bool skips(int g, int c) {
    const int t = c >> 1, dy = t / 3 - 1, dx = t % 3 - 1;
    return g == G0 ? dy < 0 : g == G0 + 1 ? dy > 0 : g == G0 + 2 ? dx < 0 : g == G0 + 3 ? dx > 0 : false;
  }
  static constexpr unsigned active(int c) {
    unsigned m = 0;
    for (int g = 0; g < NG; ++g) m |= (skips(g, c) ? 0u : 1u) << g;
    return m;
  }
  static constexpr unsigned first(int c) {
    unsigned m = active(c);
    for (int k = 0; k < c; ++k) m &= ~active(k);
    return m;
  }
  static constexpr int pos0(int c) {
    int n = 0;
    for (int k = 0; k < c; ++k)
      for (int g = 0; g < NG; ++g) n += skips(g, k) ? 0 : 1;
    return n;
  }
};
// the map is a bijection onto the board's pixels
template <int N>
constexpr bool ln_edge_map_is_bijection() {
  constexpr int RS = ln_row(N), NG = ln_groups(N);
  const LnEdgePixMap<N> m{};
  bool seen[N * N] = {};
  for (int i = 0; i < NG * 16; ++i) {
    const int sl = m.slot[i];
    if (sl < 0) return false;
    const int r = sl / RS - 1, c = sl % RS - 1;
    if (r < 0 || r >= N || c < 0 || c >= N || seen[r * N + c]) return false;
    seen[r * N + c] = true;
  }
  return true;
}
// every pair the schedule skips reads only cells off the board (the zero halo) in all 16 columns;
// every group runs in some chunk (its INIT), and the groups the ring reads ahead across a chunk
// boundary (the first kLnPf) run in every chunk
template <int N>
constexpr bool ln_edge_sched_skips_only_halo() {
  using S = LnEdgeSched<N>;
  constexpr int RS = ln_row(N);
  const LnEdgePixMap<N> m{};
  unsigned ran = 0;
  for (int c = 0; c < S::NC; ++c) {
    const int t = c >> 1, dy = t / 3 - 1, dx = t % 3 - 1;
    if ((S::active(c) & ((1u << kLnPf) - 1u)) != (1u << kLnPf) - 1u) return false;
    ran |= S::active(c);
    for (int g = 0; g < S::NG; ++g) {
      if (!S::skips(g, c)) continue;
      for (int n = 0; n < 16; ++n) {
        const int sl = m.slot[g * 16 + n], r = sl / RS - 1 + dy, col = sl % RS - 1 + dx;
        if (r >= 0 && r < N && col >= 0 && col < N) return false;
      }
    }
  }
  return ran == (1u << S::NG) - 1u;
}

template <int N>
__device__ __forceinline__ int ln_pixel(int slot) {  // grid slot -> board pixel index
  return (slot / ln_row(N) - 1) * N + slot % ln_row(N) - 1;
}

__device__ __forceinline__ f32x4 mfma16(h16x8 a, h16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}

// x (already scaled) -> packed f16 halves: hi = f16(x) (round to nearest), lo = f16(x - hi)
// (3 VALU ops per pair: x - hi is exact in f32 (|x - hi| <= half an f16 ulp of x), so the mix op's
// one rounding of fma(-hi, 1, x) to f16 is f16(x - hi) as a convert-back-and-subtract form
// computes it (5 ops): bitwise the same)
__device__ __forceinline__ void split2(float x0, float x1, unsigned& hi, unsigned& lo) {
  asm("v_cvt_pk_f16_f32 %0, %2, %3\n\t"
      "v_fma_mixlo_f16 %1, -%0, 1.0, %2 op_sel_hi:[1,0,0]\n\t"
      "v_fma_mixhi_f16 %1, -%0, 1.0, %3 op_sel:[1,0,0] op_sel_hi:[1,0,0]"
      : "=&v"(hi), "=&v"(lo)
      : "v"(x0), "v"(x1));
}

__device__ __forceinline__ f32x2 pk_fma(f32x2 a, f32x2 b, f32x2 c) {
  f32x2 r;
  asm("v_pk_fma_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}
__device__ __forceinline__ f32x2 pk_add(f32x2 a, f32x2 b) {
  f32x2 r;
  asm("v_pk_add_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}

__device__ __forceinline__ f32x2 pk_sub(f32x2 a, f32x2 b) {
  f32x2 r;
  asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
// 4-wide adds / subtracts as two packed f32 ops (the compiler emits four v_sub_f32 for f32x4)
__device__ __forceinline__ f32x4 add4(f32x4 a, f32x4 b) {
  const f32x2 lo = pk_add(f32x2{a.x, a.y}, f32x2{b.x, b.y}), hi = pk_add(f32x2{a.z, a.w}, f32x2{b.z, b.w});
  return f32x4{lo.x, lo.y, hi.x, hi.y};
}
__device__ __forceinline__ f32x4 sub4(f32x4 a, f32x4 b) {
  const f32x2 lo = pk_sub(f32x2{a.x, a.y}, f32x2{b.x, b.y}), hi = pk_sub(f32x2{a.z, a.w}, f32x2{b.z, b.w});
  return f32x4{lo.x, lo.y, hi.x, hi.y};
}
__device__ __forceinline__ f32x4 fma4(f32x4 a, f32x4 b, f32x4 c) {
  const f32x2 lo = pk_fma(f32x2{a.x, a.y}, f32x2{b.x, b.y}, f32x2{c.x, c.y});
  const f32x2 hi = pk_fma(f32x2{a.z, a.w}, f32x2{b.z, b.w}, f32x2{c.z, c.w});
  return f32x4{lo.x, lo.y, hi.x, hi.y};
}

// max(m, |a|, |b|) in one VALU op (fmaxf would canonicalize every input first)
__device__ __forceinline__ float max3_abs(float m, float a, float b) {
  float r;
  asm("v_max3_f32 %0, %1, |%2|, |%3|" : "=v"(r) : "v"(m), "v"(a), "v"(b));
  return r;
}
// max(y, floor) as signed integers: y for floor = INT_MIN, relu(y) for floor = 0 (-0 -> +0),
// one v_max_i32 (the float max would add a canonicalize per input)
__device__ __forceinline__ float max_bits(float y, int floor) {
  return __builtin_bit_cast(float, max(__builtin_bit_cast(int, y), floor));
}

// a buffer resource over [p, p + bytes), its base made provably wave-uniform (readfirstlane): the
// tower's weight loads as buffer ops (a per-lane VGPR offset + a wave-uniform SGPR offset per
// chunk) instead of one 64-bit VGPR address per load
__device__ __forceinline__ __amdgpu_buffer_rsrc_t ln_rsrc(const void* p, unsigned bytes) {
  const uintptr_t a = (uintptr_t)p;
  const uintptr_t u = ((uintptr_t)(unsigned)__builtin_amdgcn_readfirstlane((int)(a >> 32)) << 32) |
                      (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)a);
  return __builtin_amdgcn_make_buffer_rsrc((void*)u, 0, (int)bytes, 0x00020000);
}

// the power of two that brings the largest magnitude m into [2^14, 2^15)
__device__ __forceinline__ int scale_exp(float m) {
  if (!(m > 0.0f) || !(m < __builtin_inff())) return 0;
  int e;
  (void)frexpf(m, &e);  // m = f 2^e, f in [0.5, 1)
  const int s = 15 - e;
  return s < -64 ? -64 : (s > 64 ? 64 : s);
}

// maximum of m over the workgroup (red: 4 floats of LDS); a barrier inside
__device__ __forceinline__ float block_max(float m, float* red, int wave, int l) {
  m = wave_max_f(m);
  if (l == 0) red[wave] = m;
  __syncthreads();
  return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// The lane's B fragments (hi, lo) of one group: grid + pb (the lane's slot in bytes) + coff (the
// chunk's plane and tap offset); HALF = byte offset of the lo halves from the hi halves.
template <int HALF>
__device__ __forceinline__ void ln_load(h16x8 (&r)[2], const unsigned char* grid, int pb, int coff) {
  const unsigned char* q = grid + pb + coff;
  r[0] = *reinterpret_cast<const h16x8*>(q);
  r[1] = *reinterpret_cast<const h16x8*>(q + HALF);
}

// Fill the ring with the first kLnPf groups of a chunk (at a layer start, after the barrier).
template <int NG, int HALF>
__device__ __forceinline__ void ln_prime(h16x8 (&rb)[kLnSlots][2], const unsigned char* grid, const int (&pb)[NG],
                                         int coff) {
#pragma unroll
  for (int g = 0; g < kLnPf; ++g) ln_load<HALF>(rb[g], grid, pb[g], coff);
}

// One K chunk over the board's NG pixel groups: acc[g] += ah*bh + al*bh + ah*bl with the group's
// B fragments from the ring, whose reads run kLnPf groups ahead and on into the next chunk
// (coff_next; on the last chunk of a layer any in-grid offset: those reads are never consumed).
// The MFMAs are inline asm with the accumulator in place (srcC = vdst: back-to-back accumulation,
// no copies; VGPRs or AGPRs per BK_LN_VACC); INIT starts the accumulators from 0.
template <int NG, bool INIT, int HALF>
__device__ __forceinline__ void ln_chunk(f32x4 (&acc)[NG], h16x8 ah, h16x8 al, const unsigned char* grid,
                                         const int (&pb)[NG], int coff, int coff_next, h16x8 (&rb)[kLnSlots][2]) {
  static_assert(NG % kLnSlots == 0, "ln_chunk: the ring slot of a group must not depend on the chunk");
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    const int gp = g + kLnPf;
    if (gp < NG)
      ln_load<HALF>(rb[gp % kLnSlots], grid, pb[gp], coff);
    else
      ln_load<HALF>(rb[gp % kLnSlots], grid, pb[gp - NG], coff_next);
    const h16x8 bh = rb[g % kLnSlots][0], bl = rb[g % kLnSlots][1];
    if (INIT)
      asm volatile(
          "v_mfma_f32_16x16x32_f16 %0, %1, %2, 0\n\t"
          "v_mfma_f32_16x16x32_f16 %0, %3, %2, %0\n\t"
          "v_mfma_f32_16x16x32_f16 %0, %1, %4, %0"
          : BK_ACC_W(acc[g])
          : "v"(ah), "v"(bh), "v"(al), "v"(bl));
    else
      asm volatile(
          "v_mfma_f32_16x16x32_f16 %0, %1, %2, %0\n\t"
          "v_mfma_f32_16x16x32_f16 %0, %3, %2, %0\n\t"
          "v_mfma_f32_16x16x32_f16 %0, %1, %4, %0"
          : BK_ACC_RW(acc[g])
          : "v"(ah), "v"(bh), "v"(al), "v"(bl));
#if BK_LN_DUMMY
    {  // timing diagnostic only: BK_LN_DUMMY independent VALU ops after each triple (the MFMA shadow)
      float d0 = __builtin_bit_cast(float, (unsigned)g), d1 = d0;
#pragma unroll
      for (int k = 0; k < BK_LN_DUMMY; ++k) {
        if (k & 1)
          asm volatile("v_add_f32 %0, %0, %0" : "+v"(d1));
        else
          asm volatile("v_add_f32 %0, %0, %0" : "+v"(d0));
      }
      asm volatile("" ::"v"(d0), "v"(d1));
    }
#endif
  }
}

// ln_prime / ln_chunk for a grid whose lo halves are identically zero (the stem on a binary
// board built from a packed state, k_leafnet_x3<N, true>): only the hi plane exists, it alone is
// read (ring entries [g][0]), and each group takes two MFMAs, acc[g] += ah*bh + al*bh, in
// ln_chunk's order. The product left out, ah*bl with bl = 0, is the last of ln_chunk's triple and
// adds exactly +-0, so every accumulator equals ln_chunk's as a float value.
template <int NG>
__device__ __forceinline__ void ln_prime_hi(h16x8 (&rb)[kLnSlots][2], const unsigned char* grid, const int (&pb)[NG],
                                            int coff) {
#pragma unroll
  for (int g = 0; g < kLnPf; ++g) rb[g][0] = *reinterpret_cast<const h16x8*>(grid + pb[g] + coff);
}
template <int NG, bool INIT>
__device__ __forceinline__ void ln_chunk_hi(f32x4 (&acc)[NG], h16x8 ah, h16x8 al, const unsigned char* grid,
                                            const int (&pb)[NG], int coff, int coff_next, h16x8 (&rb)[kLnSlots][2]) {
  static_assert(NG % kLnSlots == 0, "ln_chunk_hi: the ring slot of a group must not depend on the chunk");
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    const int gp = g + kLnPf;
    rb[gp % kLnSlots][0] = *reinterpret_cast<const h16x8*>(grid + (gp < NG ? pb[gp] + coff : pb[gp - NG] + coff_next));
    const h16x8 bh = rb[g % kLnSlots][0];
    if (INIT)
      asm volatile(
          "v_mfma_f32_16x16x32_f16 %0, %1, %2, 0\n\t"
          "v_mfma_f32_16x16x32_f16 %0, %3, %2, %0"
          : BK_ACC_W(acc[g])
          : "v"(ah), "v"(bh), "v"(al));
    else
      asm volatile(
          "v_mfma_f32_16x16x32_f16 %0, %1, %2, %0\n\t"
          "v_mfma_f32_16x16x32_f16 %0, %3, %2, %0"
          : BK_ACC_RW(acc[g])
          : "v"(ah), "v"(bh), "v"(al));
  }
}

// ln_chunk with each group's two B-fragment reads (kLnPf groups ahead) issued between its three
// MFMAs in one asm block: wait (lgkmcnt(2 (kLnPf - 1)): the reads of the kLnPf - 1 blocks before
// are the only ones still allowed in flight), MFMA, read hi, MFMA, read lo, MFMA — one instruction in each MFMA's
// issue gap instead of two reads and a wait in one (a 16x16x32 MFMA holds the SIMD's issue for 8
// of its 16 cycles: MI355X_MICROARCH.md). The reads are invisible to the compiler: the grid offsets
// must be compile-time constants (immediates), the ring registers are only read by later blocks
// (after their wait), and the caller waits lgkmcnt(0) after its last chunk, before the ring
// registers can be reused. Same MFMAs on the same operands as ln_chunk: the sums are bitwise equal.
template <int NG, bool INIT, int HALF>
__device__ __forceinline__ void ln_chunk_il(f32x4 (&acc)[NG], h16x8 ah, h16x8 al, const unsigned char* grid,
                                            const int (&pb)[NG], int coff, int coff_next, h16x8 (&rb)[kLnSlots][2]) {
  static_assert(NG % kLnSlots == 0, "ln_chunk_il: the ring slot of a group must not depend on the chunk");
  const unsigned gbase = (unsigned)(uintptr_t)grid;
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    const int gp = g + kLnPf;
    const unsigned addr = gbase + (unsigned)(gp < NG ? pb[gp] : pb[gp - NG]);
    h16x8& n0 = rb[gp % kLnSlots][0];
    h16x8& n1 = rb[gp % kLnSlots][1];
    if (gp < NG) {
      if (INIT)
        asm volatile(
            "s_waitcnt lgkmcnt(%10)\n\t"
            "v_mfma_f32_16x16x32_f16 %0, %3, %5, 0\n\t"
            "ds_read_b128 %1, %7 offset:%8\n\t"
            "v_mfma_f32_16x16x32_f16 %0, %4, %5, %0\n\t"
            "ds_read_b128 %2, %7 offset:%9\n\t"
            "v_mfma_f32_16x16x32_f16 %0, %3, %6, %0"
            : BK_ACC_W(acc[g]), "=&v"(n0), "=&v"(n1)
            : "v"(ah), "v"(al), "v"(rb[g % kLnSlots][0]), "v"(rb[g % kLnSlots][1]), "v"(addr), "i"(coff), "i"(coff + HALF), "i"(2 * (kLnPf - 1)));
      else
        asm volatile(
            "s_waitcnt lgkmcnt(%10)\n\t"
            "v_mfma_f32_16x16x32_f16 %0, %3, %5, %0\n\t"
            "ds_read_b128 %1, %7 offset:%8\n\t"
            "v_mfma_f32_16x16x32_f16 %0, %4, %5, %0\n\t"
            "ds_read_b128 %2, %7 offset:%9\n\t"
            "v_mfma_f32_16x16x32_f16 %0, %3, %6, %0"
            : BK_ACC_RW(acc[g]), "=&v"(n0), "=&v"(n1)
            : "v"(ah), "v"(al), "v"(rb[g % kLnSlots][0]), "v"(rb[g % kLnSlots][1]), "v"(addr), "i"(coff), "i"(coff + HALF), "i"(2 * (kLnPf - 1)));
    } else {
      if (INIT)
        asm volatile(
            "s_waitcnt lgkmcnt(%10)\n\t"
            "v_mfma_f32_16x16x32_f16 %0, %3, %5, 0\n\t"
            "ds_read_b128 %1, %7 offset:%8\n\t"
            "v_mfma_f32_16x16x32_f16 %0, %4, %5, %0\n\t"
            "ds_read_b128 %2, %7 offset:%9\n\t"
            "v_mfma_f32_16x16x32_f16 %0, %3, %6, %0"
            : BK_ACC_W(acc[g]), "=&v"(n0), "=&v"(n1)
            : "v"(ah), "v"(al), "v"(rb[g % kLnSlots][0]), "v"(rb[g % kLnSlots][1]), "v"(addr), "i"(coff_next),
              "i"(coff_next + HALF), "i"(2 * (kLnPf - 1)));
      else
        asm volatile(
            "s_waitcnt lgkmcnt(%10)\n\t"
            "v_mfma_f32_16x16x32_f16 %0, %3, %5, %0\n\t"
            "ds_read_b128 %1, %7 offset:%8\n\t"
            "v_mfma_f32_16x16x32_f16 %0, %4, %5, %0\n\t"
            "ds_read_b128 %2, %7 offset:%9\n\t"
            "v_mfma_f32_16x16x32_f16 %0, %3, %6, %0"
            : BK_ACC_RW(acc[g]), "=&v"(n0), "=&v"(n1)
            : "v"(ah), "v"(al), "v"(rb[g % kLnSlots][0]), "v"(rb[g % kLnSlots][1]), "v"(addr), "i"(coff_next),
              "i"(coff_next + HALF), "i"(2 * (kLnPf - 1)));
    }
  }
}

// The groups a chunk runs (bit mask ACT), in order, then the next chunk's first kLnPf groups as
// NG + g (the ring reads on into them; they run in every chunk).
template <int NG, unsigned ACT>
struct LnActive {
  int n;
  int g[NG + kLnPf];
  constexpr LnActive() : n(0), g() {
    for (int k = 0; k < NG; ++k)
      if ((ACT >> k) & 1u) g[n++] = k;
    for (int k = 0; k < kLnPf; ++k) g[n + k] = NG + k;
  }
};

// ln_chunk_il over the chunk's active groups only (LnEdgeSched): ACT the groups it runs, INIT those
// of them that start their accumulator here, POS0 the layer's count of active (chunk, group) pairs
// before this chunk. The ring slot of a pair is its position in that sequence mod kLnSlots (not
// g % kLnSlots: the chunks differ in length); ln_prime fills positions 0..kLnPf-1. Each block
// reads the pair kLnPf positions ahead, in this chunk or the next one's first groups. A group
// left out keeps its accumulator: the products left out are a*0, whose sum +-0 changes no
// accumulator that started at +0 and received only MFMA sums (never -0), so the sums are bitwise
// ln_chunk_il's. Same lgkmcnt discipline: the wait inside each block, the caller's lgkmcnt(0)
// after the last chunk, the ring registers written only by the asm blocks.
template <int NG, unsigned ACT, unsigned INIT, int POS0, int HALF>
__device__ __forceinline__ void ln_chunk_il_act(f32x4 (&acc)[NG], h16x8 ah, h16x8 al, const unsigned char* grid,
                                                const int (&pb)[NG], int coff, int coff_next,
                                                h16x8 (&rb)[kLnSlots][2]) {
  constexpr LnActive<NG, ACT> A{};
  static_assert((INIT & ~ACT) == 0u && A.n >= kLnPf, "ln_chunk_il_act: INIT groups run; the ring fits the chunk");
  const unsigned gbase = (unsigned)(uintptr_t)grid;
#pragma unroll
  for (int i = 0; i < A.n; ++i) {
    const int g = A.g[i], gp = A.g[i + kLnPf];
    const int s = (POS0 + i) % kLnSlots, sp = (POS0 + i + kLnPf) % kLnSlots;
    const unsigned addr = gbase + (unsigned)(gp < NG ? pb[gp] : pb[gp - NG]);
    h16x8& n0 = rb[sp][0];
    h16x8& n1 = rb[sp][1];
    if (gp < NG) {
      if ((INIT >> g) & 1u)
        asm volatile(
            "s_waitcnt lgkmcnt(%10)\n\t"
            "v_mfma_f32_16x16x32_f16 %0, %3, %5, 0\n\t"
            "ds_read_b128 %1, %7 offset:%8\n\t"
            "v_mfma_f32_16x16x32_f16 %0, %4, %5, %0\n\t"
            "ds_read_b128 %2, %7 offset:%9\n\t"
            "v_mfma_f32_16x16x32_f16 %0, %3, %6, %0"
            : BK_ACC_W(acc[g]), "=&v"(n0), "=&v"(n1)
            : "v"(ah), "v"(al), "v"(rb[s][0]), "v"(rb[s][1]), "v"(addr), "i"(coff), "i"(coff + HALF), "i"(2 * (kLnPf - 1)));
      else
        asm volatile(
            "s_waitcnt lgkmcnt(%10)\n\t"
            "v_mfma_f32_16x16x32_f16 %0, %3, %5, %0\n\t"
            "ds_read_b128 %1, %7 offset:%8\n\t"
            "v_mfma_f32_16x16x32_f16 %0, %4, %5, %0\n\t"
            "ds_read_b128 %2, %7 offset:%9\n\t"
            "v_mfma_f32_16x16x32_f16 %0, %3, %6, %0"
            : BK_ACC_RW(acc[g]), "=&v"(n0), "=&v"(n1)
            : "v"(ah), "v"(al), "v"(rb[s][0]), "v"(rb[s][1]), "v"(addr), "i"(coff), "i"(coff + HALF), "i"(2 * (kLnPf - 1)));
    } else {
      if ((INIT >> g) & 1u)
        asm volatile(
            "s_waitcnt lgkmcnt(%10)\n\t"
            "v_mfma_f32_16x16x32_f16 %0, %3, %5, 0\n\t"
            "ds_read_b128 %1, %7 offset:%8\n\t"
            "v_mfma_f32_16x16x32_f16 %0, %4, %5, %0\n\t"
            "ds_read_b128 %2, %7 offset:%9\n\t"
            "v_mfma_f32_16x16x32_f16 %0, %3, %6, %0"
            : BK_ACC_W(acc[g]), "=&v"(n0), "=&v"(n1)
            : "v"(ah), "v"(al), "v"(rb[s][0]), "v"(rb[s][1]), "v"(addr), "i"(coff_next), "i"(coff_next + HALF),
              "i"(2 * (kLnPf - 1)));
      else
        asm volatile(
            "s_waitcnt lgkmcnt(%10)\n\t"
            "v_mfma_f32_16x16x32_f16 %0, %3, %5, %0\n\t"
            "ds_read_b128 %1, %7 offset:%8\n\t"
            "v_mfma_f32_16x16x32_f16 %0, %4, %5, %0\n\t"
            "ds_read_b128 %2, %7 offset:%9\n\t"
            "v_mfma_f32_16x16x32_f16 %0, %3, %6, %0"
            : BK_ACC_RW(acc[g]), "=&v"(n0), "=&v"(n1)
            : "v"(ah), "v"(al), "v"(rb[s][0]), "v"(rb[s][1]), "v"(addr), "i"(coff_next), "i"(coff_next + HALF),
              "i"(2 * (kLnPf - 1)));
    }
  }
}

// f(integral_constant<int, 0>{}) ... f(integral_constant<int, NC - 1>{}): a chunk loop whose index
// is a compile-time value (ln_chunk_il_act's schedule arguments)
template <class F, int... Cs>
__device__ __forceinline__ void ln_each_chunk(F&& f, std::integer_sequence<int, Cs...>) {
  (f(std::integral_constant<int, Cs>{}), ...);
}

// the accumulators are written by MFMAs the compiler cannot see: wait out the MFMA write ->
// VALU read latency before the epilogue reads them. Each accumulator then passes through an empty
// asm that follows the wait (volatile asm keeps its order), so no read of it can be scheduled
// above the wait (an 8-wave variant of this kernel read one too early without this).
template <int NG>
__device__ __forceinline__ void ln_mfma_drain(f32x4 (&acc)[NG]) {
  asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 7" ::: "memory");
#pragma unroll
  for (int g = 0; g < NG; ++g) asm volatile("" : BK_ACC_RW(acc[g]));
}

struct LnHeads {
  const float *wp, *bp, *wv, *bv, *w1t, *b1, *w2, *b2;
  int P;
  float* pf;
  float* v;
};

// The rows form of the packed-state input (bk_leafnet_x3_rows): workgroup r evaluates the state
// row tree[r] with the weight set nets[net[r]], or returns at once when the row is not live at
// `sim`, its seat is uninformed or its tree has no leaf for the net. The weight sets travel as
// kernel arguments and are picked by a wave-uniform index (scalar selects: the MFMA loop sees the
// same scalar pointers as the single-net kernels).
constexpr int kLnMaxNets = BK_ARENA_MAX_NETS;
struct LnNet {
  const h16x8* wstem;
  const float *sstem, *bstem;
  const h16x8* wt;
  const float *st, *bt, *bounds;
  const float *wp, *bp, *wv, *bv, *w1t, *b1, *w2, *b2;
};
struct LnRows {
  const uint32_t* states;
  const int32_t* status;
  const int32_t *tree, *net, *sims;
  int sim, nnets, ntrees;
  LnNet nets[kLnMaxNets];
};
__device__ __forceinline__ LnNet ln_pick(const LnNet (&n)[kLnMaxNets], int k) {
  LnNet o;
#define BK_LN_PICK(f) o.f = k == 0 ? n[0].f : k == 1 ? n[1].f : k == 2 ? n[2].f : n[3].f
  BK_LN_PICK(wstem);
  BK_LN_PICK(sstem);
  BK_LN_PICK(bstem);
  BK_LN_PICK(wt);
  BK_LN_PICK(st);
  BK_LN_PICK(bt);
  BK_LN_PICK(bounds);
  BK_LN_PICK(wp);
  BK_LN_PICK(bp);
  BK_LN_PICK(wv);
  BK_LN_PICK(bv);
  BK_LN_PICK(w1t);
  BK_LN_PICK(b1);
  BK_LN_PICK(w2);
  BK_LN_PICK(b2);
#undef BK_LN_PICK
  return o;
}
// the kernel's weight set from the C-ABI's operands
inline LnNet ln_net_of(const bk_leafnet_args& a) {
  return LnNet{reinterpret_cast<const h16x8*>(a.wstem), a.sstem, a.bstem,
               reinterpret_cast<const h16x8*>(a.wtower), a.stower, a.btower, a.bounds,
               a.wp, a.bp, a.wv, a.bv, a.w1t, a.b1, a.w2, a.b2};
}
// the heads of w writing rows t0.. of a's pf and vout (the rows form: an empty w and t0 = 0, the
// kernel takes the row's weights from its table and its outputs go to the row's tree)
inline LnHeads ln_heads_of(const bk_leafnet_args& a, const LnNet& w, int t0) {
  return LnHeads{w.wp, w.bp, w.wv, w.bv, w.w1t, w.b1, w.w2, w.b2, a.P, a.pf + (size_t)t0 * 2 * a.N * a.N,
                 a.vout + (size_t)t0 * a.P};
}
// the packed-state input (LnStates / NpStates) at row t0 of a's states and status
template <typename S>
inline S ln_states_of(const bk_leafnet_args& a, int t0) {
  return S{reinterpret_cast<const uint32_t*>(a.states) + (size_t)t0 * kStateWords, a.status ? a.status + t0 : nullptr};
}
// the kernel's table from the C-ABI's (validated by bk_leafnet_x3_rows)
inline LnRows ln_rows_of(const bk_leafnet_args* nets, int nnets, const bk_arena_rows* rows, int sim) {
  LnRows in{};
  in.states = reinterpret_cast<const uint32_t*>(nets[0].states);
  in.status = nets[0].status;
  in.tree = rows->tree_of_row;
  in.net = rows->net_of_row;
  in.sims = rows->sims_of_row;
  in.sim = sim;
  in.nnets = nnets;
  in.ntrees = rows->T;
  for (int k = 0; k < nnets; ++k) in.nets[k] = ln_net_of(nets[k]);
  return in;
}
// the row's tree and weight set, or -1 (workgroup-uniform) when the row has nothing to evaluate
__device__ __forceinline__ int ln_row_tree(const LnRows& in, int r, int& k) {
  const int t = __builtin_amdgcn_readfirstlane(in.tree[r]);
  k = -1;
  if (t < 0 || t >= in.ntrees || in.sim >= __builtin_amdgcn_readfirstlane(in.sims[r])) return -1;
  k = __builtin_amdgcn_readfirstlane(in.net[r]);
  if (k < 0 || k >= in.nnets) return -1;
  return __builtin_amdgcn_readfirstlane(in.status[t]) == 1 ? t : -1;
}

}  // namespace
}  // namespace bk

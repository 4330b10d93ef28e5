// dcnnheads.hip — DCNNet's heads for the leaf evaluator (nets.LeafDCNNet, dcnn_leaf "fused"): the
// crop of the fourth convolution's full-frame NHWC output [B][N][N][128] to its interior
// [2:N-2, 2:N-2], fc1 (K1 = 128 (N-4)^2 -> 128) + bias + ReLU, fc2 (128 -> 64) + bias + ReLU (the
// features the search's sparse policy head reads) and v = tanh(fc4 (64 -> P) + bias), BatchNorm
// folded into fc1 / fc2 (nets.fold_dcnn). Two launches:
//
// k_dcnn_fc1<PXS>: fc1 split along K into S slices of PXS consecutive interior pixels of one row
// (PXS x 128 contiguous floats of a board; S and PXS depend on N only: HeadGeom). A workgroup takes
// one slice of a tile of 64 boards (16 at 7x7): it stages the tile's slice in LDS once (the interior is read
// straight out of the full frame: no crop copy, and nothing outside the interior is touched), then
// its four waves each compute 32 of the 128 outputs for all the tile's boards on the exact-f32 MFMA
// (v_mfma_f32_16x16x4_f32: A = weights, B = activations, one MFMA column per board, so a board's
// sums depend neither on its batch nor on its place in it). The weights stream from global memory
// in fragment order (bk_dcnn_heads_pack): 1 KB per wave load, every weight read once per tile.
// The slice's partial sums go to the workspace [S][B][128].
//
// k_dcnn_tail: one workgroup per board adds the S partial sums in slice order (no atomics), then
// bias, ReLU, fc2, ReLU, fc4 and tanh in fp32 (fmaf chains in index order).
#include "../../include/blokus_engine.h"
#include "ctx.h"

#include <type_traits>

#include "leafnet_common.h"

namespace bk {
namespace {

// boards per workgroup tile (MFMA column blocks of 16): 64, or 16 where a slice is one pixel (7x7:
// 9 slices only, so the small tile is what spreads a batch over the CUs)
__host__ __device__ constexpr int head_boards(int pxs) { return pxs == 1 ? 16 : 64; }

// the K split of an N x N board: slices of PXS pixels of one interior row
struct HeadGeom {
  int M, pxs, S, KC;
};
__host__ inline HeadGeom head_geom(int N) {
  const int M = N - 4, pxs = N == 20 ? 4 : N == 14 ? 2 : 1;  // 16 / 10 / 3 pixels per row
  return HeadGeom{M, pxs, M * M / pxs, pxs * 128};
}

// fragment order of fc1's weights: float4 index ((s * KS + ks) * 8 + blk) * 64 + lane, KS = KC / 16;
// element e of lane (i = lane & 15, q = lane >> 4) = w[16 blk + i][s KC + q KC / 4 + 4 ks + e]
// (the quarter q of the slice at a distance of KC / 4 floats: the LDS reads of the four quarters
// then fall on the same banks only across the lane groups of a ds_read_b128)
__global__ __launch_bounds__(256) void k_dcnn_heads_pack(const float* __restrict__ w, float* __restrict__ wp, int K1,
                                                         int KC) {
  const long long n = 128LL * K1;
  const int KS = KC / 16;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const int e = (int)(i & 3), lane = (int)((i >> 2) & 63), blk = (int)((i >> 8) & 7);
    const long long sk = i >> 11;  // s * KS + ks
    const int s = (int)(sk / KS), ks = (int)(sk - (long long)s * KS);
    const int o = 16 * blk + (lane & 15), q = lane >> 4;
    wp[i] = w[(size_t)o * K1 + (size_t)s * KC + q * (KC / 4) + 4 * ks + e];
  }
}

template <int PXS>
__global__ __launch_bounds__(256) void k_dcnn_fc1(const float* __restrict__ x, const f32x4* __restrict__ wp,
                                                     float* __restrict__ ws, int B, int N) {
  constexpr int KC = PXS * 128, RS = KC + 4, KS = KC / 16, Q4 = KC / 4;
  constexpr int kHeadBoards = head_boards(PXS), NBB = kHeadBoards / 16;
  constexpr int PF = 4;  // weight steps in flight (a step's 32 MFMAs are ~0.4 us: below the L2 / HBM latency)
  static_assert(KS % PF == 0, "k_dcnn_fc1: the weight ring is unrolled whole");
  extern __shared__ __attribute__((aligned(16))) float act[];  // [64 boards][RS]: row stride = 4 mod 64 dwords
  const int tid = threadIdx.x, M = N - 4;
  const int s = blockIdx.x, b0 = blockIdx.y * kHeadBoards, nb = min(kHeadBoards, B - b0);
  const int pi = s * PXS, r = pi / M, col = pi - r * M;  // the slice's first interior pixel
  const size_t poff = ((size_t)(r + 2) * N + col + 2) * 128, bstride = (size_t)N * N * 128;
  const int l = tid & 63, j = l & 15, q = l >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const f32x4* wsrc = wp + ((size_t)s * KS * 8 + 2 * wave) * 64 + l;
  f32x4 wr[PF][2];  // the ring: step ks in slot ks % PF
#pragma unroll
  for (int p = 0; p < PF; ++p) {
    wr[p][0] = wsrc[(size_t)p * 512];
    wr[p][1] = wsrc[(size_t)p * 512 + 64];
  }
  // the tile's slice into LDS: all of a thread's loads (at most 32 float4) in flight before its writes
  constexpr int NST = kHeadBoards * Q4 / 256, CH = NST < 32 ? NST : 32;
  static_assert(NST >= 1 && NST % CH == 0, "k_dcnn_fc1: staging steps");
  for (int i0 = 0; i0 < NST; i0 += CH) {
    f32x4 v[CH];
#pragma unroll
    for (int u = 0; u < CH; ++u) {
      const int i = (i0 + u) * 256 + tid, bd = i / Q4, q4 = i - bd * Q4;
      v[u] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (bd < nb) v[u] = *reinterpret_cast<const f32x4*>(x + (size_t)(b0 + bd) * bstride + poff + 4 * q4);
    }
#pragma unroll
    for (int u = 0; u < CH; ++u) {
      const int i = (i0 + u) * 256 + tid, bd = i / Q4, q4 = i - bd * Q4;
      *reinterpret_cast<f32x4*>(&act[bd * RS + 4 * q4]) = v[u];
    }
  }
  __syncthreads();
  const int nbb = (nb + 15) >> 4;  // live board blocks of the tile
  f32x4 acc[2][NBB];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int bb = 0; bb < NBB; ++bb) acc[h][bb] = f32x4{0.f, 0.f, 0.f, 0.f};
  const float* arow = act + j * RS + q * Q4;
  // a full tile runs the loop without the per-block tests (one basic block per step: the LDS reads
  // are scheduled ahead of the MFMAs); a part tile skips its empty blocks
  auto run = [&](auto full_c) {
    constexpr bool FULL = decltype(full_c)::value;
    for (int k0 = 0; k0 < KS; k0 += PF) {
#pragma unroll
      for (int p = 0; p < PF; ++p) {
        const int ks = k0 + p;
        const f32x4 a0 = wr[p][0], a1 = wr[p][1];
        const int kn = ks + PF < KS ? ks + PF : ks;  // (the last steps reload their own: no read past the slice)
        wr[p][0] = wsrc[(size_t)kn * 512];
        wr[p][1] = wsrc[(size_t)kn * 512 + 64];
#pragma unroll
        for (int bb = 0; bb < NBB; ++bb) {
          if (FULL || bb < nbb) {
            const f32x4 bv = *reinterpret_cast<const f32x4*>(arow + bb * 16 * RS + 4 * ks);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              acc[0][bb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[e], bv[e], acc[0][bb], 0, 0, 0);
              acc[1][bb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[e], bv[e], acc[1][bb], 0, 0, 0);
            }
          }
        }
      }
    }
  };
  if (nbb == NBB)
    run(std::true_type{});
  else
    run(std::false_type{});
  // D: lane (j, q) holds outputs 16 blk + 4 q .. + 3 of board 16 bb + j
#pragma unroll
  for (int bb = 0; bb < NBB; ++bb) {
    const int bd = 16 * bb + j;
    if (bd >= nb) continue;
    float* dst = ws + ((size_t)s * B + b0 + bd) * 128 + 32 * wave + 4 * q;
    *reinterpret_cast<f32x4*>(dst) = acc[0][bb];
    *reinterpret_cast<f32x4*>(dst + 16) = acc[1][bb];
  }
}

__global__ __launch_bounds__(128) void k_dcnn_tail(const float* __restrict__ ws, int S, int B, int P,
                                                   const float* __restrict__ b1, const float* __restrict__ w2t,
                                                   const float* __restrict__ b2, const float* __restrict__ w4t,
                                                   const float* __restrict__ b4, float* __restrict__ feats,
                                                   float* __restrict__ v) {
  __shared__ float h1[128], h2[64];
  const int t = threadIdx.x, b = blockIdx.x;
  // every weight a thread needs, loaded before the partial sums (one trip to the L2 in all)
  float w2[128], w4[64];
  const int t2 = t & 63, t4 = t < P ? t : 0;
#pragma unroll
  for (int k = 0; k < 128; ++k) w2[k] = w2t[k * 64 + t2];
#pragma unroll
  for (int k = 0; k < 64; ++k) w4[k] = w4t[k * P + t4];
  const float bb1 = b1[t], bb2 = b2[t2], bb4 = b4[t4];
  float a = 0.0f;
  const float* src = ws + (size_t)b * 128 + t;
  int s = 0;
  for (; s + 8 <= S; s += 8) {  // in slice order, eight loads in flight
    float p[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) p[i] = src[(size_t)(s + i) * B * 128];
#pragma unroll
    for (int i = 0; i < 8; ++i) a += p[i];
  }
  for (; s < S; ++s) a += src[(size_t)s * B * 128];
  a += bb1;
  h1[t] = a < 0.0f ? 0.0f : a;
  __syncthreads();
  if (t < 64) {
    float c = 0.0f;
#pragma unroll
    for (int k = 0; k < 128; ++k) c = fmaf(h1[k], w2[k], c);
    c += bb2;
    c = c < 0.0f ? 0.0f : c;
    h2[t] = c;
    feats[(size_t)b * 64 + t] = c;
  }
  __syncthreads();
  if (t < P) {
    float c = 0.0f;
#pragma unroll
    for (int k = 0; k < 64; ++k) c = fmaf(h2[k], w4[k], c);
    v[(size_t)b * P + t] = tanhf(c + bb4);
  }
}

__host__ inline bool a16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

template <int PXS>
int launch_fc1(const float* x, const float* wp, float* ws, int B, int N, int S, hipStream_t s) {
  constexpr int kHeadBoards = head_boards(PXS);
  constexpr int lds = kHeadBoards * (PXS * 128 + 4) * 4;
  static_assert(lds <= 160 * 1024, "k_dcnn_fc1: LDS");
  {
    const void* fns[1] = {(const void*)k_dcnn_fc1<PXS>};
    if (set_max_dynamic_lds(fns, 1, lds) != BK_OK) return BK_EHIP;
  }
  const dim3 grid((unsigned)S, (unsigned)((B + kHeadBoards - 1) / kHeadBoards));
  hipLaunchKernelGGL(k_dcnn_fc1<PXS>, grid, dim3(256), lds, s, x, (const f32x4*)wp, ws, B, N);
  return launch_check("k_dcnn_fc1");
}

}  // namespace
}  // namespace bk

using namespace bk;

extern "C" {

int bk_dcnn_heads_supported(int N) { return N == 7 || N == 14 || N == 20; }

int bk_dcnn_heads_slices(int N) { return bk_dcnn_heads_supported(N) ? head_geom(N).S : 0; }

int bk_dcnn_heads_weight_floats(int N) { return bk_dcnn_heads_supported(N) ? 128 * 128 * (N - 4) * (N - 4) : 0; }

int bk_dcnn_heads_pack(const float* fc1_w, int N, float* packed, void* stream) {
  BK_REQUIRE(fc1_w && packed, "bad argument");
  BK_REQUIRE(bk_dcnn_heads_supported(N), "bk_dcnn_heads_pack: board size must be 7, 14 or 20");
  const HeadGeom g = head_geom(N);
  const int K1 = 128 * g.M * g.M;
  const long long n = 128LL * K1;
  const int grid = (int)((n + 255) / 256 < 2048 ? (n + 255) / 256 : 2048);
  hipLaunchKernelGGL(k_dcnn_heads_pack, dim3(grid), dim3(256), 0, (hipStream_t)stream, fc1_w, packed, K1, g.KC);
  return launch_check("k_dcnn_heads_pack");
}

int bk_dcnn_heads(const float* x, int B, int N, int P, const float* fc1_packed, const float* fc1_b, const float* fc2_wt,
                  const float* fc2_b, const float* fc4_wt, const float* fc4_b, float* workspace, float* feats,
                  float* v, void* stream) {
  BK_REQUIRE(fc1_packed && fc1_b && fc2_wt && fc2_b && fc4_wt && fc4_b && B >= 0, "bad argument");
  BK_REQUIRE(B == 0 || (x && workspace && feats && v), "bad argument");
  BK_REQUIRE(bk_dcnn_heads_supported(N), "bk_dcnn_heads: board size must be 7, 14 or 20");
  BK_REQUIRE(P >= 1 && P <= 64, "bk_dcnn_heads: 1 to 64 value outputs");
  BK_REQUIRE(a16(x) && a16(fc1_packed) && a16(workspace), "bk_dcnn_heads: 16-byte aligned buffers");
  if (B == 0) return BK_OK;
  const HeadGeom g = head_geom(N);
  hipStream_t s = (hipStream_t)stream;
  const int rc = g.pxs == 4   ? launch_fc1<4>(x, fc1_packed, workspace, B, N, g.S, s)
                 : g.pxs == 2 ? launch_fc1<2>(x, fc1_packed, workspace, B, N, g.S, s)
                              : launch_fc1<1>(x, fc1_packed, workspace, B, N, g.S, s);
  if (rc != BK_OK) return rc;
  hipLaunchKernelGGL(k_dcnn_tail, dim3(B), dim3(128), 0, s, workspace, g.S, B, P, fc1_b, fc2_wt, fc2_b, fc4_wt, fc4_b,
                     feats, v);
  return launch_check("k_dcnn_tail");
}

}  // extern "C"

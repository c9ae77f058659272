// The grouped skinny GEMM of the routed experts over block-scaled FP8 tables (include/ssd_hip_moe_fp8b.h): the grouped walk of
// moe.hip -- a workgroup owns one expert and one span of 16-row groups and walks that expert's perm range in MFMA tiles of 16 token
// rows, the B operand gathered from row-major activations -- over the checkpoint's own e4m3 codes and fp32 block scales.
//
// The unit of work is the 128-column BLOCK, because that is the unit of the scale:
//  * codes: a block of a 16-row group is 2 KiB, two adjacent 1 KiB k-pairs of the fp8 frag layout, so a lane's A operand is two
//    16-byte loads; fp8x8_to_bf16 (exact, scale operand 1.0) widens them into the A slices of four v_mfma_f32_16x16x32_bf16 k-steps;
//  * the four k-steps go into a ZEROED fp32 temporary, then acc = fma(s, temporary, acc): one fma per block and accumulator
//    register.  The temporaries cost NT * MT * 4 VGPRs beside the accumulators;
//  * the scale is one fp32 per (16-row group, block): uniform over the wave, read through the scalar cache with a wave-uniform
//    address (blockIdx, the wave index through readfirstlane, the block counter) and held in an SGPR;
//  * K is dealt to the waves in whole blocks (wave v: blocks v, v + W, ...), so a block's temporary and scale live in one wave.
//    W = 2 below 8 blocks, 4 from 8 on: a function of K alone, part of the normative accumulation order.
// What is sized for the 2 KiB-per-block stream: a wave issues the loads of U of its blocks (codes, scales and, up to two token
// tiles, the token operands) before the first conversion waits.  A block costs 8 VGPRs per row group against mxfp4's 4, so the same U
// holds twice the bytes: 4 for a gate / up pair at one token tile (16 KiB in flight per wave, a wave's whole share of K = 2048),
// 3 for four down groups at one token tile (24 KiB, the whole share of K = 768), 2 elsewhere.  At four token tiles the token
// operands are loaded per block, from L2.
// A pass covers 16 * MT token rows; an expert with more rows (long prefills) takes several passes and reads its codes once per pass.
#include "common.h"
#include "gemm_fp8.h"
#include "ssd_hip_moe_fp8b.h"

// grid (spans of NT 16-row groups of the table, E); W waves per workgroup
template <int EPI, int NT, int MT, int W, int U>
__global__ void __launch_bounds__(W * 64)
moe_fp8b_gemm_kernel(const bf16_t* __restrict__ X, const u32x4_t* __restrict__ Qf, const float* __restrict__ Sg,
                     const int32_t* __restrict__ offs, const int32_t* __restrict__ perm, bf16_t* __restrict__ out, int T, int k, int N,
                     int K) {
  static_assert(EPI != SSD_MOE_EPI_UP || NT == 2, "one gate / up pair per workgroup");
  constexpr bool XS = MT <= 2;                                 // the token operands ride with the batch's loads
  __shared__ f32x4_t red[W][NT * MT][64];
  const int e = blockIdx.y;
  const int n_ent = T * k;
  int r0 = offs[e], r1 = offs[e + 1];
  r0 = min(max(r0, 0), n_ent);
  r1 = min(max(r1, r0), n_ent);
  if (r0 >= r1) return;                                        // nobody chose this expert: its tables are not read
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int KB = K >> 7, NG = N >> 4;
  const int g0 = blockIdx.x * NT;
  const int gv = min(NT, NG - g0);                             // groups of this span that exist (the last span of a down table)
  const size_t qstride = (size_t)KB << 7;                      // 16-byte chunks between adjacent row groups: 2 KiB per block
  const u32x4_t* qp = Qf + ((size_t)e * NG + g0) * qstride + lane;
  const float* sp = Sg + ((size_t)e * NG + g0) * KB;           // wave-uniform
  const int mcol = lane & 15, nrow = (lane >> 4) * 4;
  const int ldo = EPI == SSD_MOE_EPI_UP ? (N >> 1) : N;
  for (int rb = r0; rb < r1; rb += 16 * MT) {
    const int mtv = min(MT, (r1 - rb + 15) >> 4);              // row tiles of this pass that hold an entry (wave-uniform)
    int ent[MT];
    const bf16_t* xr[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const int i = rb + mt * 16 + mcol;
      int en = i < r1 ? perm[i] : -1;
      if (en < 0 || en >= n_ent) en = -1;
      ent[mt] = en;
      const int row = EPI == SSD_MOE_EPI_UP ? en / k : en;
      xr[mt] = X + (size_t)(en < 0 ? 0 : row) * K + (lane >> 4) * 8;
    }
    // the lane's 8 columns of k-tile 4c + j of token tile mt (zeros for a column of the tile without an entry)
    auto xload = [&](int mt, int c, int j) {
      u32x4_t v = {0u, 0u, 0u, 0u};
      if (ent[mt] >= 0) v = *reinterpret_cast<const u32x4_t*>(xr[mt] + (size_t)c * 128 + j * 32);
      return v;
    };
    f32x4_t acc[NT][MT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) acc[nt][mt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    // wave v: blocks v, v + W, ... in ascending order, U of them per batch (c < KB is wave-uniform)
    for (int c0 = wave; c0 < KB; c0 += U * W) {
      u32x4_t a[U][NT][2], b[U][XS ? MT : 1][4];
      float s[U][NT];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int c = c0 + u * W;
        if (c < KB) {
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) {
            const int g = nt < gv ? nt : 0;
            const u32x4_t* p = qp + g * qstride + ((size_t)c << 7);
            a[u][nt][0] = __builtin_nontemporal_load(p);        // k-tiles 4c, 4c + 1
            a[u][nt][1] = __builtin_nontemporal_load(p + 64);   // k-tiles 4c + 2, 4c + 3
            s[u][nt] = sp[(size_t)g * KB + c];
          }
          if (XS) {
#pragma unroll
            for (int mt = 0; mt < (XS ? MT : 1); ++mt)
#pragma unroll
              for (int j = 0; j < 4; ++j) b[u][mt][j] = xload(mt, c, j);
          }
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int c = c0 + u * W;
        if (c < KB) {
          u32x4_t w[NT][4];
#pragma unroll
          for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int j = 0; j < 4; ++j) w[nt][j] = fp8x8_to_bf16(a[u][nt][j >> 1][(j & 1) * 2], a[u][nt][j >> 1][(j & 1) * 2 + 1]);
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) {
            if (mt >= mtv) continue;
            u32x4_t bj[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) bj[j] = XS ? b[u][XS ? mt : 0][j] : xload(mt, c, j);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
              f32x4_t t = {0.f, 0.f, 0.f, 0.f};                 // the block's own sum, from +0
#pragma unroll
              for (int j = 0; j < 4; ++j) t = mfma16(w[nt][j], bj[j], t);
#pragma unroll
              for (int r = 0; r < 4; ++r) acc[nt][mt][r] = __builtin_fmaf(s[u][nt], t[r], acc[nt][mt][r]);
            }
          }
        }
      }
    }
    // ---- the W waves' partial sums through LDS, added in wave order ----
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) red[wave][nt * MT + mt][lane] = acc[nt][mt];
    __syncthreads();
    if (EPI == SSD_MOE_EPI_UP) {
      // groups (0, 1) of the span = (gate, up) of features 16 blockIdx.x ..: silu(g) * u on the bf16-rounded values, one rounding
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        if ((mt & (W - 1)) != wave || mt >= mtv) continue;
        f32x4_t g = red[0][mt][lane], u = red[0][MT + mt][lane];
#pragma unroll
        for (int v = 1; v < W; ++v) {
          g += red[v][mt][lane];
          u += red[v][MT + mt][lane];
        }
        float o[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float gb = round_bf(g[r]), ub = round_bf(u[r]);
          o[r] = (gb / (1.0f + __expf(-gb))) * ub;
        }
        if (ent[mt] >= 0)
          *reinterpret_cast<u32x2_t*>(out + (size_t)ent[mt] * ldo + blockIdx.x * 16 + nrow) = u32x2_t{pack_bf2(o[0], o[1]), pack_bf2(o[2], o[3])};
      }
    } else {
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          if (((nt * MT + mt) & (W - 1)) != wave || mt >= mtv || nt >= gv) continue;
          f32x4_t sum = red[0][nt * MT + mt][lane];
#pragma unroll
          for (int v = 1; v < W; ++v) sum += red[v][nt * MT + mt][lane];
          if (ent[mt] >= 0)
            *reinterpret_cast<u32x2_t*>(out + (size_t)ent[mt] * ldo + (g0 + nt) * 16 + nrow) = u32x2_t{pack_bf2(sum[0], sum[1]), pack_bf2(sum[2], sum[3])};
        }
    }
    if (rb + 16 * MT < r1) __syncthreads();                    // the next pass overwrites red
  }
}

template <int EPI, int NT, int MT, int U>
static void moe_fp8b_launch(const void* rows_in, const void* q_frag, const float* s_grp, const int32_t* offs, const int32_t* perm, void* out,
                            int T, int k, int E, int N, int K, hipStream_t stream) {
  const dim3 grid((unsigned)(((N >> 4) + NT - 1) / NT), (unsigned)E);
  // the normative wave count: 2 below 8 blocks of K, 4 from 8 on
  if ((K >> 7) >= 8)
    hipLaunchKernelGGL((moe_fp8b_gemm_kernel<EPI, NT, MT, 4, U>), grid, dim3(256), 0, stream, (const bf16_t*)rows_in, (const u32x4_t*)q_frag,
                       s_grp, offs, perm, (bf16_t*)out, T, k, N, K);
  else
    hipLaunchKernelGGL((moe_fp8b_gemm_kernel<EPI, NT, MT, 2, U>), grid, dim3(128), 0, stream, (const bf16_t*)rows_in, (const u32x4_t*)q_frag,
                       s_grp, offs, perm, (bf16_t*)out, T, k, N, K);
}

extern "C" int ssd_moe_gemm_fp8b(const void* rows_in, const void* q_frag, const float* s_grp, const int32_t* offs, const int32_t* perm,
                                 void* out, int T, int k, int E, int N, int K, int epilogue, void* stream) {
  if (!rows_in || !q_frag || !s_grp || !offs || !perm || !out) return SSD_ERR_ARG;
  if (epilogue != SSD_MOE_EPI_UP && epilogue != SSD_MOE_EPI_DOWN) return SSD_ERR_ARG;
  if (T <= 0 || k < 1 || k > SSD_MOE_MAX_K || E < SSD_MOE_MIN_E || E > SSD_MOE_MAX_E || (E & 7) || k > E) return SSD_ERR_SHAPE;
  if ((long)T * k > (1L << 24)) return SSD_ERR_SHAPE;
  if (K <= 0 || (K & 127) || N <= 0) return SSD_ERR_SHAPE;
  if (epilogue == SSD_MOE_EPI_UP ? (N & 63) : (N & 15)) return SSD_ERR_SHAPE;
  // an expert holds at most T rows (a token names an expert once): the row tiles per pass follow from T alone
  const int mt = T <= 16 ? 1 : T <= 32 ? 2 : 4;
  hipStream_t st = (hipStream_t)stream;
#define MOE_F8B(EPI, NT, MT, U) moe_fp8b_launch<EPI, NT, MT, U>(rows_in, q_frag, s_grp, offs, perm, out, T, k, E, N, K, st)
  if (epilogue == SSD_MOE_EPI_UP) {
    if (mt == 1) MOE_F8B(SSD_MOE_EPI_UP, 2, 1, 4); else if (mt == 2) MOE_F8B(SSD_MOE_EPI_UP, 2, 2, 2); else MOE_F8B(SSD_MOE_EPI_UP, 2, 4, 2);
  } else {
    if (mt == 1) MOE_F8B(SSD_MOE_EPI_DOWN, 4, 1, 3); else if (mt == 2) MOE_F8B(SSD_MOE_EPI_DOWN, 4, 2, 2); else MOE_F8B(SSD_MOE_EPI_DOWN, 2, 4, 2);
  }
#undef MOE_F8B
  return hipGetLastError() == hipSuccess ? SSD_OK : SSD_ERR_LAUNCH;
}

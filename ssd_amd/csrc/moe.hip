// Routed mixture-of-experts MLP (include/ssd_hip_moe.h): top-k routing with its grouping tables, the grouped skinny GEMM over the
// experts' fragment-major tables, and the weighted combine.
//
// The GEMM is the hot path.  A verify of 8 rows touches up to 64 experts, each with a handful of token rows, so the launch is a
// weight stream like gemm_wf_kernel's: a workgroup owns one expert and one span of output features, its 4 waves split K and every
// table byte of a chosen expert is read once per 16 * MT token rows.  The MFMA operand roles are those of the dense GEMMs: the A
// operand is the table (16 table rows -> D rows), the B operand is the token tile (16 token rows -> D columns), so a token row only
// ever influences its own D column and the padding columns of a ragged tile compute values that are never stored.  The B operand is
// gathered from ROW-MAJOR activations (lane l reads 16 bytes of row perm[..] at column 32 kt + 8 (l >> 4)): the rows of an expert are
// scattered over the batch, and a fragment-major image of them would have to be rebuilt per expert.
#include "common.h"
#include "ssd_hip_moe.h"

constexpr int MOE_WAVES = 4;        // waves per workgroup of every kernel here

// ---- routing ---------------------------------------------------------------------------------------------------------------------
struct MoeCand { float v; int i; };
__device__ __forceinline__ MoeCand moe_better(MoeCand a, MoeCand b) {       // larger value, then lower index
  return (b.v > a.v || (b.v == a.v && b.i < a.i)) ? b : a;
}

// one wave per token row; lane l holds experts l, l + 64, l + 128, l + 192
__global__ void __launch_bounds__(MOE_WAVES * 64)
moe_topk_kernel(const bf16_t* __restrict__ logits, long ld, int T, int E, int k, int norm, int32_t* __restrict__ ids,
                float* __restrict__ w) {
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * MOE_WAVES + (threadIdx.x >> 6);
  if (t >= T) return;
  const bf16_t* row = logits + (size_t)t * ld;
  float v[4], c[4], p[4];
  float m = -INFINITY;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int e = lane + 64 * i;
    v[i] = e < E ? bf2f(row[e]) : -INFINITY;
    c[i] = v[i] != v[i] ? -INFINITY : v[i];        // the key of the selection: a NaN never wins against a number
    if (c[i] > m) m = c[i];
  }
  m = wave_max(m);
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    p[i] = lane + 64 * i < E ? expf(v[i] - m) : 0.f;
    s += p[i];
  }
  s = wave_sum(s);
  unsigned taken = 0;
  int my_id = 0;
  float my_p = 0.f;
  for (int j = 0; j < k; ++j) {
    MoeCand b = {-INFINITY, 0x7fffffff};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = lane + 64 * i;
      if (e < E && !((taken >> i) & 1u)) b = moe_better(b, MoeCand{c[i], e});
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) b = moe_better(b, MoeCand{__shfl_xor(b.v, o, 64), __shfl_xor(b.i, o, 64)});
    const int slot = b.i >> 6, owner = b.i & 63;
    float pw = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (i == slot) pw = p[i];
    pw = __shfl(pw, owner, 64) / s;
    if (lane == owner) taken |= 1u << slot;
    if (lane == j) { my_id = b.i; my_p = pw; }
  }
  if (norm) {
    float den = 0.f;
    for (int j = 0; j < k; ++j) den += __shfl(my_p, j, 64);
    my_p = my_p / den;
  }
  if (lane < k) {
    ids[(size_t)t * k + lane] = my_id;
    w[(size_t)t * k + lane] = round_bf(my_p);
  }
}

// one workgroup per expert walks the n = T * k ids twice: the entries below it give offs[e], the entries equal to it are written to
// perm in ascending entry order (ballot + prefix over the 4 waves per strip of 256 entries)
__global__ void __launch_bounds__(MOE_WAVES * 64)
moe_group_kernel(const int32_t* __restrict__ ids, int n, int E, int32_t* __restrict__ offs, int32_t* __restrict__ perm) {
  __shared__ int wcnt[MOE_WAVES];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int e = blockIdx.x;
  int less = 0;
  for (int i = threadIdx.x; i < n; i += MOE_WAVES * 64) less += ids[i] < e ? 1 : 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) less += __shfl_xor(less, o, 64);
  if (lane == 0) wcnt[wave] = less;
  __syncthreads();
  int run = 0;
#pragma unroll
  for (int v = 0; v < MOE_WAVES; ++v) run += wcnt[v];
  const int base = run;
  __syncthreads();
  for (int s0 = 0; s0 < n; s0 += MOE_WAVES * 64) {
    const int i = s0 + threadIdx.x;
    const bool hit = i < n && ids[i] == e;
    const unsigned long long bal = __ballot(hit);
    const int before = __popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) wcnt[wave] = __popcll(bal);
    __syncthreads();
    int pre = 0, tot = 0;
#pragma unroll
    for (int v = 0; v < MOE_WAVES; ++v) {
      if (v < wave) pre += wcnt[v];
      tot += wcnt[v];
    }
    const int dst = run + pre + before;
    if (hit && dst < n) perm[dst] = i;
    run += tot;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    offs[e] = base;
    if (e == E - 1) offs[E] = run;
  }
}

// ---- the grouped skinny GEMM -------------------------------------------------------------------------------------------------------
// grid (spans of NT 16-row groups of the table, E).  Workgroup (s, e) multiplies groups NT s .. of expert e's table with the rows of
// perm[offs[e] .. offs[e + 1]), 16 * MT rows per pass.
template <int EPI, int NT, int MT>
__global__ void __launch_bounds__(MOE_WAVES * 64)
moe_gemm_kernel(const bf16_t* __restrict__ X, const u32x4_t* __restrict__ Wf, const int32_t* __restrict__ offs,
                const int32_t* __restrict__ perm, bf16_t* __restrict__ out, int T, int k, int N, int K) {
  __shared__ f32x4_t red[MOE_WAVES][NT * MT][64];
  const int e = blockIdx.y;
  const int n_ent = T * k;
  int r0 = offs[e], r1 = offs[e + 1];
  r0 = min(max(r0, 0), n_ent);
  r1 = min(max(r1, r0), n_ent);
  if (r0 >= r1) return;                                        // nobody chose this expert: its table is not read
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int KT = K >> 5, NG = N >> 4;
  const int g0 = blockIdx.x * NT;
  const int gv = min(NT, NG - g0);                             // groups of this span that exist (the last span of a down table)
  const size_t wstride = (size_t)KT << 6;                      // chunks between adjacent row groups
  const u32x4_t* wp = Wf + ((size_t)e * NG + g0) * wstride + lane;
  const int mcol = lane & 15, nrow = (lane >> 4) * 4;
  const int ldo = EPI == SSD_MOE_EPI_UP ? (N >> 1) : N;
  constexpr int U = (NT + MT <= 4) ? 4 : 2;                    // k-tiles whose loads are all in flight before the first MFMA waits
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
    f32x4_t acc[NT][MT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) acc[nt][mt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    // wave v: k-tiles v, v + 4, ... in ascending order
    int kt = wave;
    for (; kt + (U - 1) * MOE_WAVES < KT; kt += U * MOE_WAVES) {
      u32x4_t a[U][NT], b[U][MT];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int kk = kt + u * MOE_WAVES;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) a[u][nt] = __builtin_nontemporal_load(wp + (nt < gv ? nt : 0) * wstride + ((size_t)kk << 6));
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          u32x4_t v = {0u, 0u, 0u, 0u};
          if (ent[mt] >= 0) v = *reinterpret_cast<const u32x4_t*>(xr[mt] + (size_t)kk * 32);
          b[u][mt] = v;
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
          for (int mt = 0; mt < MT; ++mt)
            if (mt < mtv) acc[nt][mt] = mfma16(a[u][nt], b[u][mt], acc[nt][mt]);
    }
    for (; kt < KT; kt += MOE_WAVES) {
      u32x4_t a[NT];
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) a[nt] = __builtin_nontemporal_load(wp + (nt < gv ? nt : 0) * wstride + ((size_t)kt << 6));
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        u32x4_t v = {0u, 0u, 0u, 0u};
        if (ent[mt] >= 0) v = *reinterpret_cast<const u32x4_t*>(xr[mt] + (size_t)kt * 32);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
          if (mt < mtv) acc[nt][mt] = mfma16(a[nt], v, acc[nt][mt]);
      }
    }
    // ---- the 4 waves' partial sums through LDS, added in wave order ----
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) red[wave][nt * MT + mt][lane] = acc[nt][mt];
    __syncthreads();
    if (EPI == SSD_MOE_EPI_UP) {
      // groups (0, 1) of the span = (gate, up) of features 16 blockIdx.x ..: silu(g) * u on the bf16-rounded values, one rounding
      static_assert(EPI != SSD_MOE_EPI_UP || NT == 2, "one gate / up pair per workgroup");
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        if ((mt & (MOE_WAVES - 1)) != wave || mt >= mtv) continue;
        f32x4_t g = red[0][mt][lane], u = red[0][MT + mt][lane];
#pragma unroll
        for (int v = 1; v < MOE_WAVES; ++v) {
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
          if (((nt * MT + mt) & (MOE_WAVES - 1)) != wave || mt >= mtv || nt >= gv) continue;
          f32x4_t s = red[0][nt * MT + mt][lane];
#pragma unroll
          for (int v = 1; v < MOE_WAVES; ++v) s += red[v][nt * MT + mt][lane];
          if (ent[mt] >= 0)
            *reinterpret_cast<u32x2_t*>(out + (size_t)ent[mt] * ldo + (g0 + nt) * 16 + nrow) = u32x2_t{pack_bf2(s[0], s[1]), pack_bf2(s[2], s[3])};
        }
    }
    if (rb + 16 * MT < r1) __syncthreads();                    // the next pass overwrites red
  }
}

// ---- combine -----------------------------------------------------------------------------------------------------------------------
// one thread per 8 columns of a token row
__global__ void __launch_bounds__(256)
moe_combine_kernel(const u32x4_t* __restrict__ d, const float* __restrict__ w, u32x4_t* __restrict__ h, int T, int k, int H8) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)T * H8) return;
  const size_t t = i / H8, c = i % H8;
  float acc[8];
#pragma unroll
  for (int r = 0; r < 8; ++r) acc[r] = 0.f;
  for (int j = 0; j < k; ++j) {
    const float wj = w[t * k + j];
    const u32x4_t v = d[(t * k + j) * H8 + c];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      acc[2 * r] = acc[2 * r] + wj * bf2f(v[r] & 0xffffu);
      acc[2 * r + 1] = acc[2 * r + 1] + wj * bf2f(v[r] >> 16);
    }
  }
  h[i] = u32x4_t{pack_bf2(acc[0], acc[1]), pack_bf2(acc[2], acc[3]), pack_bf2(acc[4], acc[5]), pack_bf2(acc[6], acc[7])};
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
static int moe_check(int T, int k, int E) {
  if (T <= 0 || k < 1 || k > SSD_MOE_MAX_K || E < SSD_MOE_MIN_E || E > SSD_MOE_MAX_E || (E & 7) || k > E) return SSD_ERR_SHAPE;
  if ((long)T * k > (1L << 24)) return SSD_ERR_SHAPE;
  return SSD_OK;
}

extern "C" int ssd_moe_route(const void* logits_rows, long ld, int T, int E, int k, int norm, int32_t* topk_ids, float* topk_w,
                             int32_t* offs, int32_t* perm, void* stream) {
  if (!logits_rows || !topk_ids || !topk_w || !offs || !perm) return SSD_ERR_ARG;
  const int rc = moe_check(T, k, E);
  if (rc != SSD_OK) return rc;
  if (ld < E) return SSD_ERR_SHAPE;
  hipLaunchKernelGGL(moe_topk_kernel, dim3((unsigned)((T + MOE_WAVES - 1) / MOE_WAVES)), dim3(MOE_WAVES * 64), 0, (hipStream_t)stream,
                     (const bf16_t*)logits_rows, ld, T, E, k, norm, topk_ids, topk_w);
  hipLaunchKernelGGL(moe_group_kernel, dim3((unsigned)E), dim3(MOE_WAVES * 64), 0, (hipStream_t)stream, (const int32_t*)topk_ids, T * k, E,
                     offs, perm);
  return hipGetLastError() == hipSuccess ? SSD_OK : SSD_ERR_LAUNCH;
}

extern "C" int ssd_moe_gemm(const void* rows_in, const void* w_frag, const int32_t* offs, const int32_t* perm, void* out, int T, int k,
                            int E, int N, int K, int epilogue, void* stream) {
  if (!rows_in || !w_frag || !offs || !perm || !out) return SSD_ERR_ARG;
  if (epilogue != SSD_MOE_EPI_UP && epilogue != SSD_MOE_EPI_DOWN) return SSD_ERR_ARG;
  const int rc = moe_check(T, k, E);
  if (rc != SSD_OK) return rc;
  if (K <= 0 || (K & 31) || N <= 0) return SSD_ERR_SHAPE;
  if (epilogue == SSD_MOE_EPI_UP ? (N & 63) : (N & 15)) return SSD_ERR_SHAPE;
  // an expert holds at most T rows (a token names an expert once): the row tiles per pass follow from T alone
  const int mt = T <= 16 ? 1 : T <= 32 ? 2 : 4;
  const int NG = N >> 4;
#define MOE_GEMM(EPI, NT, MT)                                                                                                      \
  hipLaunchKernelGGL((moe_gemm_kernel<EPI, NT, MT>), dim3((unsigned)((NG + NT - 1) / NT), (unsigned)E), dim3(MOE_WAVES * 64), 0,     \
                     (hipStream_t)stream, (const bf16_t*)rows_in, (const u32x4_t*)w_frag, offs, perm, (bf16_t*)out, T, k, N, K)
  if (epilogue == SSD_MOE_EPI_UP) {
    if (mt == 1) MOE_GEMM(SSD_MOE_EPI_UP, 2, 1); else if (mt == 2) MOE_GEMM(SSD_MOE_EPI_UP, 2, 2); else MOE_GEMM(SSD_MOE_EPI_UP, 2, 4);
  } else {
    if (mt == 1) MOE_GEMM(SSD_MOE_EPI_DOWN, 4, 1); else if (mt == 2) MOE_GEMM(SSD_MOE_EPI_DOWN, 4, 2); else MOE_GEMM(SSD_MOE_EPI_DOWN, 2, 4);
  }
#undef MOE_GEMM
  return hipGetLastError() == hipSuccess ? SSD_OK : SSD_ERR_LAUNCH;
}

extern "C" int ssd_moe_combine(const void* d_rows, const float* topk_w, void* h_rows, int T, int k, int H, void* stream) {
  if (!d_rows || !topk_w || !h_rows) return SSD_ERR_ARG;
  if (T <= 0 || k < 1 || k > SSD_MOE_MAX_K || H <= 0 || (H & 15) || (long)T * k > (1L << 24)) return SSD_ERR_SHAPE;
  const size_t items = (size_t)T * (H >> 3);
  hipLaunchKernelGGL(moe_combine_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const u32x4_t*)d_rows,
                     topk_w, (u32x4_t*)h_rows, T, k, H >> 3);
  return hipGetLastError() == hipSuccess ? SSD_OK : SSD_ERR_LAUNCH;
}

// The skeleton of the weight-quantized ("wq") skinny GEMMs: y = x . W^T with bf16 activations and a quantized W streamed once.
// gemm_fp8.hip, gemm_w4a16.hip (symmetric and zero-point) and gemm_mxfp4.hip each give a policy struct F and build their kernels
// from wq_gemm_kernel; what is written here once is the walk they share:
//  * codes are stored in 1 KiB units per (16-row group, K unit of F::KT k-tiles): one 16-byte lane load, one contiguous 1 KiB
//    wave load, F::KT MFMA k-steps.  They go straight to VGPRs with non-temporal loads.
//  * U = K units per stage and wave (the code bytes in flight per wave are U * NT KiB); K is dealt to the waves in runs of U units
//    round-robin, the < U left-over units go to the last wave (gemm_wf_kernel's walk, gemm.hip).
//  * XS: the x operands ride in the double-buffered stage; without, F::group loads them per unit (from L2: x is shared by every
//    workgroup) where the stage would not fit the VGPR budget.
//  * one workgroup owns NT row groups for the whole K; its waves split K and combine through LDS in a fixed order (deterministic).
//  * the bias, a per-row scale where the format has one, and SiLU are applied to the fp32 sums in the epilogue.
// A policy F holds only what differs between formats:
//   KSHIFT, KT        log2 of the columns of a K unit, and its k-tiles (64 / 2 for fp8, 128 / 4 for the 4-bit formats)
//   Side<MT, NT>      the side-band a stage carries next to the codes (nothing; scales; scales and zero points)
//   Band              the side-band's pointers, strides and lane offset: load(stage, nt, ku), advance(NT)
//   group()           one stage's codes -> MFMA operands -> the accumulators
//   ROW_SCALE         the epilogue multiplies the sum by a per-row fp32 scale (the s argument)
//   HAS_Z             the z argument is required
//   FORMS             (MT, nt, deep) -> (U, XS)
#pragma once
#include "common.h"

enum { WQ_ROWS = SSD_EPI_ROWS, WQ_SILU_FRAG = SSD_EPI_SILU_FRAG };

static inline int grid_for(long total) {
  long blocks = (total + 255) / 256;
  return (int)(blocks > 65536 ? 65536 : blocks);
}

// whole 16-row groups and whole K units of `kunit` (a power of two) columns
static inline bool wq_shape_ok(int N, int K, int kunit) { return N > 0 && K > 0 && (N & 15) == 0 && (K & (kunit - 1)) == 0; }

// One stage element: codes, side-band, x operands, in the order the three kernels had before they shared this header (the order
// reaches the register allocator: with the side-band first, four mxfp4 kernels came out 6 VGPRs higher).
template <int NT>
struct WqCodes {
  u32x4_t a[NT];                      // the codes of one K unit per lane and row group
};
template <class F, int MT, int NT, bool XS>
struct WqStage : WqCodes<NT>, F::template Side<MT, NT> {
  u32x4_t b[XS ? MT : 1][F::KT];      // x operands of the unit's k-tiles
};

// Sf: the scales in the format's form (F::Band reads them; with ROW_SCALE the epilogue does).  Zf: zero points, null without HAS_Z.
template <class F, int MT, int NT, int EPI, int U, bool XS>
__global__ void __launch_bounds__(512)
wq_gemm_kernel(const u32x4_t* __restrict__ Qf, const void* __restrict__ Sf, const u32x4_t* __restrict__ Xf,
               const bf16_t* __restrict__ bias, void* __restrict__ Yv, int M, int N, int K, int ldy, int tpw, const void* __restrict__ Zf) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  using Stage = WqStage<F, MT, NT, XS>;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nw = blockDim.x >> 6;
  const int KU = K >> F::KSHIFT, KT = K >> 5;
  const int ntiles = (N / 16) / NT;
  const int t_begin = blockIdx.x * tpw, t_end = min(ntiles, t_begin + tpw);
  const u32x4_t* xp = Xf + lane;
  const size_t wstride = (size_t)KU << 6;   // 16-byte chunks between adjacent row groups of q
  const size_t xstride = (size_t)KT << 6;   // 16-byte chunks between adjacent token tiles of x
  const int kstep = nw * U;
  const int ku0 = wave * U;
  const int kmain = (KU / U) * U;
  const u32x4_t* wp = Qf + ((size_t)t_begin * NT * wstride) + lane;
  typename F::Band band(Sf, Zf, (size_t)t_begin * NT, KU, lane);
  const float* scale = reinterpret_cast<const float*>(Sf);   // ROW_SCALE only
  const int mt_last = (M - 1) >> 4;
  auto xload = [&](int mt, int kt) -> u32x4_t {
    // token rows >= M of the last 16-row tile are padding: their lanes do not load; m-tiles past the last one re-read it
    u32x4_t b = {0u, 0u, 0u, 0u};
    if (NT > 1 || mt * 16 + (lane & 15) < M) b = xp[(mt < mt_last ? mt : mt_last) * xstride + ((size_t)kt << 6)];
    return b;
  };
  auto xgroup = [&](u32x4_t (&b)[XS ? MT : 1][F::KT], int ku) {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int j = 0; j < F::KT; ++j) b[mt][j] = xload(mt, F::KT * ku + j);
  };
  auto load = [&](auto& s, int ku) {   // s: Stage[U], or Stage[1] in the K remainder
    constexpr int UN = sizeof(s) / sizeof(s[0]);
#pragma unroll
    for (int u = 0; u < UN; ++u) {
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        s[u].a[nt] = __builtin_nontemporal_load(wp + nt * wstride + ((size_t)(ku + u) << 6));
        band.load(s[u], nt, ku + u);
      }
      if constexpr (XS) xgroup(s[u].b, ku + u);
    }
  };
  Stage cur[U], nxt[U];
  if (t_begin < t_end && ku0 < kmain) load(cur, ku0);

  for (int tile = t_begin; tile < t_end; ++tile) {
    const int tile0 = tile * NT;
    f32x4_t acc[NT][MT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) acc[nt][mt] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    auto compute = [&](Stage (&s)[U], int ku) {
#pragma unroll
      for (int u = 0; u < U; ++u) F::template group<MT, NT, XS>(acc, s[u], ku + u, xload, band);
    };

    int ku = ku0;
    if (ku < kmain) {
      for (; ku + kstep < kmain; ku += kstep) {
        load(nxt, ku + kstep);
        compute(cur, ku);
#pragma unroll
        for (int u = 0; u < U; ++u) cur[u] = nxt[u];
      }
      compute(cur, ku);
    }
    for (ku = (wave == nw - 1) ? kmain : KU; ku < KU; ++ku) {   // K remainder (< U units): last wave
      Stage r[1];
      load(r, ku);
      F::template group<MT, NT, XS>(acc, r[0], ku, xload, band);
    }

    // next tile: advance the weight pointers and put its first loads in flight before the combine
    wp += (size_t)NT * wstride;
    band.advance(NT);
    if (tile + 1 < t_end && ku0 < kmain) load(cur, ku0);

    // ---- cross-wave split-K combine through LDS, fixed order ----
    f32x4_t* red = reinterpret_cast<f32x4_t*>(smem);  // [nw][NT*MT][64]
    constexpr int ITEMS = NT * MT;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) red[((wave * ITEMS) + nt * MT + mt) * 64 + lane] = acc[nt][mt];
    __syncthreads();

    const int mcol = lane & 15;        // D column j -> token row m
    const int nrow = (lane >> 4) * 4;  // D rows nrow + r -> output feature n
    if (EPI == WQ_SILU_FRAG) {
      constexpr int PAIRS = NT / 2;
      const int KT2 = (N >> 1) >> 5;
      u32x2_t* out = reinterpret_cast<u32x2_t*>(Yv);
      for (int item = wave; item < PAIRS * MT; item += nw) {
        const int pr = item / MT, mt = item % MT;
        f32x4_t g = f32x4_t{0.f, 0.f, 0.f, 0.f}, u = g;
        for (int w = 0; w < nw; ++w) {
          g += red[((w * ITEMS) + (2 * pr) * MT + mt) * 64 + lane];
          u += red[((w * ITEMS) + (2 * pr + 1) * MT + mt) * 64 + lane];
        }
        const int m = mt * 16 + mcol;
        const int ng = (tile0 + 2 * pr) * 16 + nrow, nu = (tile0 + 2 * pr + 1) * 16 + nrow;   // packed rows of gate / up
        const int n = ((tile0 >> 1) + pr) * 16 + nrow;                                       // feature index in [0, N/2)
        float o[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float gb = g[r], ub = u[r];
          if constexpr (F::ROW_SCALE) { gb = scale[ng + r] * gb; ub = scale[nu + r] * ub; }
          if (bias) { gb += bf2f(bias[ng + r]); ub += bf2f(bias[nu + r]); }
          gb = round_bf(gb); ub = round_bf(ub);
          o[r] = (gb / (1.0f + __expf(-gb))) * ub;
        }
        if (m < M) out[frag_chunk(m, n >> 3, KT2) * 2 + ((n >> 2) & 1)] = u32x2_t{pack_bf2(o[0], o[1]), pack_bf2(o[2], o[3])};
      }
    } else {
      for (int item = wave; item < ITEMS; item += nw) {
        const int nt = item / MT, mt = item % MT;
        f32x4_t s = f32x4_t{0.f, 0.f, 0.f, 0.f};
        for (int w = 0; w < nw; ++w) s += red[((w * ITEMS) + item) * 64 + lane];
        const int m = mt * 16 + mcol;
        const int n = (tile0 + nt) * 16 + nrow;
        if constexpr (F::ROW_SCALE) {
#pragma unroll
          for (int r = 0; r < 4; ++r) s[r] = scale[n + r] * s[r];
        }
        if (bias) {
#pragma unroll
          for (int r = 0; r < 4; ++r) s[r] += bf2f(bias[n + r]);
        }
        if (m < M)
          *reinterpret_cast<u32x2_t*>(reinterpret_cast<bf16_t*>(Yv) + (size_t)m * ldy + n) = u32x2_t{pack_bf2(s[0], s[1]), pack_bf2(s[2], s[3])};
      }
    }
    __syncthreads();   // the combine area is reused by the next tile
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Host side: the arguments of one call, the launcher, and the decoding and dispatch of the _cfg forms.
// ---------------------------------------------------------------------------------------------------------------------
struct WqArgs {
  const void *x, *q, *s, *z, *bias;   // z: null where the format has none
  void* y;
  int M, N, K, ldy;
};

template <class F, int MT, int NT, int EPI, int U, bool XS>
static int wq_launch(const WqArgs& a, int waves, int tpw, hipStream_t st) {
  const int ntiles = (a.N / 16) / NT;
  if (tpw < 1) tpw = 1;
  const int blocks = (ntiles + tpw - 1) / tpw;
  const size_t lds = (size_t)waves * NT * MT * 64 * sizeof(f32x4_t);
  if (lds > 64 * 1024) return SSD_ERR_ARG;
  hipLaunchKernelGGL((wq_gemm_kernel<F, MT, NT, EPI, U, XS>), dim3(blocks), dim3(waves * 64), lds, st, (const u32x4_t*)a.q, a.s,
                     (const u32x4_t*)a.x, (const bf16_t*)a.bias, a.y, a.M, a.N, a.K, a.ldy, tpw, a.z);
  return hipGetLastError() == hipSuccess ? SSD_OK : SSD_ERR_LAUNCH;
}

// one entry of F::FORMS[MT 1, 2, 4, 8][nt 1, 2, 4][plain, deep]; U = 0: the format has no such kernel
struct WqForm {
  int U;
  bool XS;
};

template <class F, int MT, int EPI, int NTI, bool DEEP>
static int wq_launch_form(const WqArgs& a, int waves, int tpw, hipStream_t st) {
  constexpr WqForm f = F::FORMS[MT == 8 ? 3 : MT >> 1][NTI][DEEP];
  if constexpr (f.U == 0 || (EPI == WQ_SILU_FRAG && NTI == 0)) return SSD_ERR_ARG;   // SILU_FRAG needs gate / up pairs of row groups
  else return wq_launch<F, MT, 1 << NTI, EPI, f.U, f.XS>(a, waves, tpw, st);
}

template <class F, int MT, int EPI>
static int wq_dispatch_nt(const WqArgs& a, int nt, bool deep, int waves, int tpw, hipStream_t st) {
  switch (nt << 1 | (int)deep) {
    case 2: return wq_launch_form<F, MT, EPI, 0, false>(a, waves, tpw, st);
    case 3: return wq_launch_form<F, MT, EPI, 0, true>(a, waves, tpw, st);
    case 4: return wq_launch_form<F, MT, EPI, 1, false>(a, waves, tpw, st);
    case 5: return wq_launch_form<F, MT, EPI, 1, true>(a, waves, tpw, st);
    case 8: return wq_launch_form<F, MT, EPI, 2, false>(a, waves, tpw, st);
    case 9: return wq_launch_form<F, MT, EPI, 2, true>(a, waves, tpw, st);
    default: return SSD_ERR_ARG;
  }
}

template <class F, int MT>
static int wq_dispatch_epi(const WqArgs& a, int epilogue, int nt, bool deep, int waves, int tpw, hipStream_t st) {
  switch (epilogue) {
    case WQ_ROWS: return wq_dispatch_nt<F, MT, WQ_ROWS>(a, nt, deep, waves, tpw, st);
    case WQ_SILU_FRAG: return wq_dispatch_nt<F, MT, WQ_SILU_FRAG>(a, nt, deep, waves, tpw, st);
    default: return SSD_ERR_ARG;
  }
}

// the _cfg form of every format: nt = row groups per workgroup | deep << 8, waves = K-split | tiles per workgroup << 8
template <class F>
static int wq_gemm_cfg(const WqArgs& a, int epilogue, int nt, int waves, void* stream) {
  if (a.M <= 0 || a.M > 128 || !wq_shape_ok(a.N, a.K, 1 << F::KSHIFT)) return SSD_ERR_SHAPE;
  if (!a.x || !a.q || !a.s || !a.y || (F::HAS_Z && !a.z)) return SSD_ERR_ARG;
  if (epilogue == WQ_ROWS && a.ldy < a.N) return SSD_ERR_SHAPE;
  const int tpw = (waves >> 8) & 0xff;
  const bool deep = (nt >> 8) & 1;
  waves &= 0xff;
  nt &= 0xff;
  if (waves < 1 || waves > 8 || (nt != 1 && nt != 2 && nt != 4) || ((a.N / 16) % nt) != 0) return SSD_ERR_ARG;
  if (epilogue == WQ_SILU_FRAG && ((nt & 1) || (a.N & 63))) return SSD_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  const int mt = (a.M + 15) / 16;
  if (mt == 1) return wq_dispatch_epi<F, 1>(a, epilogue, nt, deep, waves, tpw, st);
  if (mt == 2) return wq_dispatch_epi<F, 2>(a, epilogue, nt, deep, waves, tpw, st);
  if (mt <= 4) return wq_dispatch_epi<F, 4>(a, epilogue, nt, deep, waves, tpw, st);
  return wq_dispatch_epi<F, 8>(a, epilogue, nt, deep, waves, tpw, st);
}

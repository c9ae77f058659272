// The grouped expert GEMM in its compute-bound form (include/ssd_hip_moe_tiled.h): what gemm_lm_kernel (gemm_pf.hip) is to the dense
// prefill, for the routed experts of a long prompt.  moe.hip streams an expert's table once per 64 of its rows; at 2048 prompt rows
// an expert of the 30B shapes holds ~128 rows, at 8192 ~512, and the launch is bound by MFMA issue and L2 traffic, not by HBM bytes.
//
// A workgroup multiplies BM entries of ONE expert with BN rows of that expert's table over all of K: an LDS-tiled MFMA GEMM whose
// token operand is a gather.  Both operands reach LDS by LDS-DMA in exactly the order a lane-linear ds_read_b128 hands them to
// v_mfma_f32_16x16x32_bf16 (A = 16 table rows -> D rows, B = 16 token rows -> D columns, as in moe.hip): the table is already 1 KiB
// fragment tiles, and lane l of a token tile copies the 16 bytes moe.hip loads into its B register (row perm[..], column
// 32 kt + 8 (l >> 4)) -- the DMA's global address is per lane, its LDS address lane-linear, so the gather costs no register and no
// ds_write.  Two LDS buffers of one 64-deep K stage each, one raw s_barrier per stage (gemm_lm_kernel's pipeline).
//
// FMT = MT_MX4 is the same kernel over "mx4 frag" expert tables (include/ssd_hip_moe_tiled_mxfp4.h).  The LDS-DMA cannot widen, so the
// table operand alone goes through registers: per 128-column unit a wave holds, for each of its GW row groups, the lane's 16-byte code
// chunk and 4-byte scale quad (moe_mxfp4.hip's A-operand loads), widens two of the four code words per 64-deep stage with
// v_cvt_scalef32_pk_bf16_fp4 and writes the two k-tiles lane-linear (ds_write_b128) into the LDS slots the bf16 kernel's DMA fills.
// A unit is two stages: words 0, 1 then words 2, 3 of the codes in registers; the next unit's codes are loaded into the same registers
// right after the second half is written, ahead of that stage's MFMAs.  Everything else -- work unit, grid, prefix sum, token gather,
// MFMA loop, epilogues, clamps -- is the code below, once.
//
// FMT = MT_FP8B is the kernel over block-scaled FP8 expert tables (include/ssd_hip_moe_tiled_fp8b.h): "fp8 frag" codes and one fp32
// scale per (16-row group, 128-column block).  One 1 KiB code tile is 16 rows x 64 columns, exactly one stage of one row group, so the
// weight stage is ONE 16-byte load per lane and row group: fp8x8_to_bf16 (exact, scale operand 1.0) widens words 0, 1 into the stage's
// first k-tile and words 2, 3 into its second, one lane-linear ds_write_b128 each into the slots the bf16 DMA fills.  The scale cannot
// be folded into a bf16 weight, so it multiplies a partial sum: per stage and token tile the wave's NTW tiles go through a zeroed fp32
// temporary (two k-tiles), then acc = fma(s, temporary, acc).  The token tile is the outer loop of a stage and the k-tile the inner
// one, so only NTW temporaries are live per token tile; there are two sets, and the fmas of token tile mt are issued behind the
// MFMAs of mt + 1.  The four scales of a wave's row groups are wave-uniform and are read through the scalar cache one block ahead.
#include "common.h"
#include "mx4.h"
#include "gemm_fp8.h"
#include "ssd_hip_moe_tiled.h"
#include "ssd_hip_moe_tiled_mxfp4.h"
#include "ssd_hip_moe_tiled_fp8b.h"

typedef __attribute__((address_space(1))) void* mt_gptr_t;
typedef __attribute__((address_space(3))) void* mt_lptr_t;

// the table format of an instantiation
enum { MT_BF16 = 0, MT_MX4 = 1, MT_FP8B = 2 };

// grid (nb * spans): workgroup id -> (span, block b of the bound nb = T k / BM + E), blocks fastest.  WM x WN waves; wave (wm, wn)
// owns the span's row groups wn NTW .. + NTW and the block's token tiles wm, wm + WM, ... (dealt round-robin, so a ragged block's
// tiles spread over the wm).
// Wf: the bf16 fragment tables, or the code tables with their scales in Sf (MT_MX4: e8m0 scale quads; MT_FP8B: fp32 per group and block).
template <int EPI, int BM, int BN, int WM, int WN, int FMT>
__global__ void __launch_bounds__(64 * WM * WN, WM * WN <= 4 ? 2 : 1)
moe_tiled_kernel(const bf16_t* __restrict__ X, const u32x4_t* __restrict__ Wf, const uint32_t* __restrict__ Sf,
                 const int32_t* __restrict__ offs, const int32_t* __restrict__ perm, bf16_t* __restrict__ out, int T, int k, int E, int N,
                 int K, int nb) {
  constexpr bool MX4 = FMT == MT_MX4, F8B = FMT == MT_FP8B;
  constexpr int NW = WM * WN;
  constexpr int TW = BN / 16, TX = BM / 16, TT = TW + TX;      // fragment tiles per k-tile: table groups first, then token tiles
  constexpr int GW = TW / NW, GX = TX / NW;                    // tiles of each kind a wave stages per k-tile
  constexpr int MTW = TX / WM, NTW = TW / WN;                  // token tiles / row groups of one wave's output block
  static_assert(TW % NW == 0 && TX % NW == 0 && TX % WM == 0 && TW % WN == 0 && NTW % 2 == 0, "tile geometry");
  __shared__ u32x4_t lds[2][2][TT][64];                        // [buffer][k-tile of the stage][tile][lane]: the only LDS object
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = wave / WN, wn = wave % WN;
  const int n_ent = T * k;
  const int KT = K >> 5, NG = N >> 4;

  // XCD remap (gemm_lm_kernel's): hardware places workgroup `orig` on XCD orig % 8; give each XCD a contiguous run of ids
  const int nwg = gridDim.x, orig = blockIdx.x;
  const int q = nwg >> 3, r = nwg & 7, xcd = orig & 7;
  const int wgid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (orig >> 3);
  const int span = wgid / nb, b = wgid - span * nb;

  // ---- (expert, block) of b: lane l holds experts 4 l .. 4 l + 3, a wave-wide prefix sum of their block counts (every wave alike) ----
  int lo[5], cnt[4], tot = 0;
#pragma unroll
  for (int j = 0; j < 5; ++j) lo[j] = min(max(offs[min(4 * lane + j, E)], 0), n_ent);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    lo[j + 1] = max(lo[j + 1], lo[j]);                          // a range never ends before it starts
    cnt[j] = 4 * lane + j < E ? (lo[j + 1] - lo[j] + BM - 1) / BM : 0;
    tot += cnt[j];
  }
  int incl = tot;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int v = __shfl_up(incl, o, 64);
    if (lane >= o) incl += v;
  }
  const unsigned long long hit = __ballot(incl > b);
  if (!hit) return;                                            // a surplus workgroup of the bound: no table is touched
  const int owner = __ffsll(hit) - 1;
  int me = 0, mblk = 0, mr0 = 0, mr1 = 0, p = incl - tot;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (b >= p && b < p + cnt[j]) { me = 4 * lane + j; mblk = b - p; mr0 = lo[j]; mr1 = lo[j + 1]; }
    p += cnt[j];
  }
  const int e = __builtin_amdgcn_readfirstlane(__shfl(me, owner, 64));
  const int r1 = __builtin_amdgcn_readfirstlane(__shfl(mr1, owner, 64));
  const int rb = __builtin_amdgcn_readfirstlane(__shfl(mr0, owner, 64) + __shfl(mblk, owner, 64) * BM);
  const int rows = min(BM, r1 - rb);                           // >= 1: the block exists
  const int xtv = (rows + 15) >> 4;                            // token tiles of the block that hold an entry
  const int mtv = min(MTW, max(0, (xtv - wm + WM - 1) / WM));  // ... and how many of them are this wave's
  const int g0 = span * TW;

  // ---- staging: wave v copies row groups v GW .. and token tiles v GX .. of both k-tiles of a stage ----
  const u32x4_t* wsrc[GW];
  const uint32_t* ssrc[GW];
  const bf16_t* xsrc[GX];
#pragma unroll
  for (int i = 0; i < GW; ++i) {
    const int grp = min(g0 + wave * GW + i, NG - 1);           // groups past the table (the last span): clamped, never stored
    if constexpr (MX4) {                                       // a unit of 4 k-tiles is one code chunk and one scale quad per lane
      wsrc[i] = Wf + ((((size_t)e * NG + grp) * (KT >> 2)) << 6) + lane;
      ssrc[i] = Sf + ((((size_t)e * NG + grp) * (KT >> 2)) << 4) + (lane & 15);
    } else if constexpr (F8B) {                                // a stage of 2 k-tiles is one code chunk per lane
      wsrc[i] = Wf + ((((size_t)e * NG + grp) * (KT >> 1)) << 6) + lane;
    } else {
      wsrc[i] = Wf + ((((size_t)e * NG + grp) * KT) << 6) + lane;
    }
  }
#pragma unroll
  for (int i = 0; i < GX; ++i) {
    const int idx = min(rb + (wave * GX + i) * 16 + (lane & 15), r1 - 1);   // past the last entry: that entry's row again
    int en = perm[idx];
    if (en < 0 || en >= n_ent) en = 0;
    xsrc[i] = X + (size_t)(EPI == SSD_MOE_EPI_UP ? en / k : en) * K + (lane >> 4) * 8;
  }
  auto stage_w = [&](int kt, int buf, int ks) {                // the weight operand: fragment tiles as they lie in the table
#pragma unroll
    for (int i = 0; i < GW; ++i)
      __builtin_amdgcn_global_load_lds((mt_gptr_t)(wsrc[i] + ((size_t)kt << 6)), (mt_lptr_t)&lds[buf][ks][wave * GW + i][0], 16, 0, 0);
  };
  auto stage_x = [&](int kt, int buf, int ks) {                // the token operand: 16 bytes of every lane's gathered row
#pragma unroll
    for (int i = 0; i < GX; ++i)
      if (wave * GX + i < xtv)
        __builtin_amdgcn_global_load_lds((mt_gptr_t)(xsrc[i] + (size_t)kt * 32), (mt_lptr_t)&lds[buf][ks][TW + wave * GX + i][0], 16, 0, 0);
  };
  // MX4: the codes and scale quads of the unit being staged, and the widening of code words 2 HALF, 2 HALF + 1 into the two k-tiles
  // of a stage (K % 128 == 0: a stage is half a unit, never ragged)
  u32x4_t qc[GW];
  uint32_t sc[GW];
  auto load_q = [&](int c) {
#pragma unroll
    for (int i = 0; i < GW; ++i) {
      qc[i] = __builtin_nontemporal_load(wsrc[i] + ((size_t)c << 6));
      if constexpr (MX4) sc[i] = __builtin_nontemporal_load(ssrc[i] + ((size_t)c << 4));
    }
  };
  auto widen = [&](auto half, int buf) {
    constexpr int HALF = decltype(half)::value;
#pragma unroll
    for (int i = 0; i < GW; ++i)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) lds[buf][ks][wave * GW + i][lane] = mx4_to_bf16(qc[i][2 * HALF + ks], mx4_scale(sc[i], 2 * HALF + ks));
  };
  // FP8B: load_q(kb) takes the codes of STAGE kb, and one widening fills both k-tiles of a stage
  auto widen8 = [&](int buf) {
#pragma unroll
    for (int i = 0; i < GW; ++i)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) lds[buf][ks][wave * GW + i][lane] = fp8x8_to_bf16(qc[i][2 * ks], qc[i][2 * ks + 1]);
  };
  // FP8B: the scales of this wave's NTW row groups, wave-uniform (e, span and wave come through readfirstlane / blockIdx): block c in
  // sv, block c + 1 already requested in sn.  Groups past the table read the clamped group's scale and are never stored
  const float* sp[NTW];
  float sv[NTW], sn[NTW];
  if constexpr (F8B) {
#pragma unroll
    for (int nt = 0; nt < NTW; ++nt) {
      sp[nt] = reinterpret_cast<const float*>(Sf) + ((size_t)e * NG + min(g0 + wn * NTW + nt, NG - 1)) * (KT >> 2);
      sn[nt] = sp[nt][0];
    }
  }
  auto issue = [&](int kb, int buf) {                          // the DMA of stage kb
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int kt = 2 * kb + ks;
      if (kt < KT) {
        if constexpr (FMT == MT_BF16) stage_w(kt, buf, ks);
        stage_x(kt, buf, ks);
      }
    }
  };

  f32x4_t acc[NTW][MTW];
#pragma unroll
  for (int nt = 0; nt < NTW; ++nt)
#pragma unroll
    for (int mt = 0; mt < MTW; ++mt) acc[nt][mt] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  const int nkb = (KT + 1) >> 1;
  if constexpr (MX4 || F8B) load_q(0);
  issue(0, 0);
  if constexpr (MX4) widen(std::integral_constant<int, 0>{}, 0);
  if constexpr (F8B) {
    widen8(0);
    if (1 < nkb) load_q(1);
  }
  for (int kb = 0; kb < nkb; ++kb) {
    const int cur = kb & 1;
    // RAW: this wave's DMA of stage kb has landed, and after the barrier every wave's has.  WAR: every wave finished reading buffer
    // cur ^ 1 (stage kb - 1) before the barrier, so it may be restaged right after it.  MX4: lgkmcnt(0) is the same RAW for the widened
    // tiles' ds_writes, and vmcnt(0) also lands the next unit's codes in their registers (FP8B: the next stage's codes, and lgkmcnt(0)
    // the next block's scales).
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if constexpr (F8B) {
      // the vmcnt(0) above landed the code registers, but the compiler counts for itself: let it see them used HERE, with nothing in
      // flight, so that the widening below does not wait for the token DMA issued in between
#pragma unroll
      for (int i = 0; i < GW; ++i) asm volatile("" : "+v"(qc[i]));
    }
    if (kb + 1 < nkb) issue(kb + 1, cur ^ 1);
    if constexpr (F8B) {
      // K % 128 == 0: a stage is half a block, never ragged.  Even stages open a block: its scales, and the request for the next one's
      if (!(kb & 1)) {
        const int cn = min((kb >> 1) + 1, (KT >> 2) - 1);
#pragma unroll
        for (int nt = 0; nt < NTW; ++nt) {
          sv[nt] = sn[nt];
          sn[nt] = sp[nt][cn];
        }
      }
      u32x4_t a[2][NTW];
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int nt = 0; nt < NTW; ++nt) a[ks][nt] = lds[cur][ks][wn * NTW + nt][lane];
      f32x4_t tmp[2][NTW];                                       // the stage's own sums of token tiles mt (even) and mt (odd)
#pragma unroll
      for (int mt = 0; mt <= MTW; ++mt) {
        if (mt < MTW && mt < mtv) {
          const int xt = TW + wm + WM * min(mt, MTW - 1);
          const u32x4_t b0 = lds[cur][0][xt][lane], b1 = lds[cur][1][xt][lane];
#pragma unroll
          for (int nt = 0; nt < NTW; ++nt) tmp[mt & 1][nt] = mfma16(a[0][nt], b0, f32x4_t{0.f, 0.f, 0.f, 0.f});   // from +0
#pragma unroll
          for (int nt = 0; nt < NTW; ++nt) tmp[mt & 1][nt] = mfma16(a[1][nt], b1, tmp[mt & 1][nt]);
        }
        // behind the first token tile's MFMAs, which run on while the VALU widens: stage kb + 1 from the codes the vmcnt(0) above
        // landed; once they are written the registers take stage kb + 2's
        if (mt == 0 && kb + 1 < nkb) {
          widen8(cur ^ 1);
          if (kb + 2 < nkb) load_q(kb + 2);
        }
        // the previous token tile's fmas, under this one's MFMAs
        if (mt >= 1 && mt - 1 < mtv) {
#pragma unroll
          for (int nt = 0; nt < NTW; ++nt)
#pragma unroll
            for (int r4 = 0; r4 < 4; ++r4)
              acc[nt][mt - 1][r4] = __builtin_fmaf(sv[nt], tmp[(mt - 1) & 1][nt][r4], acc[nt][mt - 1][r4]);
        }
      }
      continue;
    }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      if (2 * kb + ks >= KT) continue;                         // an odd K / 32: the last stage holds one k-tile
      u32x4_t a[NTW], bt[MTW];
#pragma unroll
      for (int nt = 0; nt < NTW; ++nt) a[nt] = lds[cur][ks][wn * NTW + nt][lane];
#pragma unroll
      for (int mt = 0; mt < MTW; ++mt)
        if (mt < mtv) bt[mt] = lds[cur][ks][TW + wm + WM * mt][lane];
#pragma unroll
      for (int mt = 0; mt < MTW; ++mt)
        if (mt < mtv) {
#pragma unroll
          for (int nt = 0; nt < NTW; ++nt) acc[nt][mt] = mfma16(a[nt], bt[mt], acc[nt][mt]);
        }
      if constexpr (MX4) {
        // behind the first k-tile's MFMAs, which run on while the VALU widens: stage kb + 1 is the second half of this unit (kb
        // even; once it is written the registers take the next unit's codes) or the first half of the next unit (kb odd), whose
        // codes the vmcnt(0) above landed
        if (ks == 0 && kb + 1 < nkb) {
          if (kb & 1) {
            widen(std::integral_constant<int, 0>{}, cur ^ 1);
          } else {
            widen(std::integral_constant<int, 1>{}, cur ^ 1);
            if (2 * kb + 4 < KT) load_q((kb >> 1) + 1);
          }
        }
      }
    }
  }

  // ---- epilogue: every lane stores 4 consecutive features of its entry (D column lane & 15, D rows 4 (lane >> 4) ..) ----
  const int mcol = lane & 15, nrow = (lane >> 4) * 4;
  const int gn0 = g0 + wn * NTW;
  const int ldo = EPI == SSD_MOE_EPI_UP ? (N >> 1) : N;
#pragma unroll
  for (int mt = 0; mt < MTW; ++mt) {
    if (mt >= mtv) continue;
    const int i = rb + (wm + WM * mt) * 16 + mcol;
    int en = i < r1 ? perm[i] : -1;
    if (en < 0 || en >= n_ent) continue;
    bf16_t* orow = out + (size_t)en * ldo + nrow;
    if constexpr (EPI == SSD_MOE_EPI_UP) {
      // groups (2 pr, 2 pr + 1) = (gate, up) of 16 features: silu(g) * u on the bf16-rounded values, one rounding
#pragma unroll
      for (int pr = 0; pr < NTW / 2; ++pr) {
        const int gg = gn0 + 2 * pr;
        if (gg >= NG) continue;
        float o[4];
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
          const float gb = round_bf(acc[2 * pr][mt][r4]), ub = round_bf(acc[2 * pr + 1][mt][r4]);
          o[r4] = (gb / (1.0f + __expf(-gb))) * ub;
        }
        *reinterpret_cast<u32x2_t*>(orow + (gg >> 1) * 16) = u32x2_t{pack_bf2(o[0], o[1]), pack_bf2(o[2], o[3])};
      }
    } else {
#pragma unroll
      for (int nt = 0; nt < NTW; ++nt) {
        if (gn0 + nt >= NG) continue;
        const f32x4_t s = acc[nt][mt];
        *reinterpret_cast<u32x2_t*>(orow + (gn0 + nt) * 16) = u32x2_t{pack_bf2(s[0], s[1]), pack_bf2(s[2], s[3])};
      }
    }
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
template <int EPI, int BM, int BN, int WM, int WN, int FMT>
static int tiled_go(const void* rows_in, const void* w_frag, const void* s_frag, const int32_t* offs, const int32_t* perm, void* out, int T,
                    int k, int E, int N, int K, hipStream_t st) {
  // sum_e ceil(n_e / BM) <= floor(T k / BM) + E: a grid that depends on no device data
  const long nb = (long)T * k / BM + E, spans = (N + BN - 1) / BN;
  if (nb * spans > 0x7fffffffL) return SSD_ERR_SHAPE;
  hipLaunchKernelGGL((moe_tiled_kernel<EPI, BM, BN, WM, WN, FMT>), dim3((unsigned)(nb * spans)), dim3(64 * WM * WN), 0, st,
                     (const bf16_t*)rows_in, (const u32x4_t*)w_frag, (const uint32_t*)s_frag, offs, perm, (bf16_t*)out, T, k, E, N, K,
                     (int)nb);
  return hipGetLastError() == hipSuccess ? SSD_OK : SSD_ERR_LAUNCH;
}

// every entry's checks and launch; s_frag is null for bf16 tables
template <int FMT>
static int tiled_entry(const void* rows_in, const void* w_frag, const void* s_frag, const int32_t* offs, const int32_t* perm, void* out,
                       int T, int k, int E, int N, int K, int epilogue, void* stream) {
  if (!rows_in || !w_frag || (FMT != MT_BF16 && !s_frag) || !offs || !perm || !out) return SSD_ERR_ARG;
  if (epilogue != SSD_MOE_EPI_UP && epilogue != SSD_MOE_EPI_DOWN) return SSD_ERR_ARG;
  if (T <= 0 || k < 1 || k > SSD_MOE_MAX_K || E < SSD_MOE_MIN_E || E > SSD_MOE_MAX_E || (E & 7) || k > E) return SSD_ERR_SHAPE;
  if ((long)T * k > (1L << 24)) return SSD_ERR_SHAPE;
  if (K <= 0 || (K & (FMT != MT_BF16 ? 127 : 31)) || N <= 0) return SSD_ERR_SHAPE;
  if (epilogue == SSD_MOE_EPI_UP ? (N & 63) : (N & 15)) return SSD_ERR_SHAPE;
  // 128 entries x 128 table rows, 2 x 2 waves (64 KiB LDS: two workgroups per CU).  A 256 x 128 form with 4 x 2 waves was measured
  // and lost at every T (DESIGN.md "Tiled expert GEMM"): an expert's ragged last block leaves more of a larger workgroup idle
  // The mx4 form keeps that shape and the 64-deep stage: a unit is widened in two halves from codes held in registers, so LDS stays
  // 64 KiB and two workgroups share a CU (DESIGN.md "Tiled expert GEMM over MXFP4 tables")
  // The fp8b form keeps them too: one 16-byte code load per lane and row group is one stage (DESIGN.md "Tiled expert GEMM over
  // block-scaled FP8 tables")
  if (epilogue == SSD_MOE_EPI_UP)
    return tiled_go<SSD_MOE_EPI_UP, SSD_MOE_TILED_BM, SSD_MOE_TILED_BN, 2, 2, FMT>(rows_in, w_frag, s_frag, offs, perm, out, T, k, E, N, K,
                                                                                   (hipStream_t)stream);
  return tiled_go<SSD_MOE_EPI_DOWN, SSD_MOE_TILED_BM, SSD_MOE_TILED_BN, 2, 2, FMT>(rows_in, w_frag, s_frag, offs, perm, out, T, k, E, N, K,
                                                                                   (hipStream_t)stream);
}

extern "C" int ssd_moe_gemm_tiled(const void* rows_in, const void* w_frag, const int32_t* offs, const int32_t* perm, void* out, int T,
                                  int k, int E, int N, int K, int epilogue, void* stream) {
  return tiled_entry<MT_BF16>(rows_in, w_frag, nullptr, offs, perm, out, T, k, E, N, K, epilogue, stream);
}

extern "C" int ssd_moe_gemm_tiled_mxfp4(const void* rows_in, const void* q_frag, const void* s_frag, const int32_t* offs,
                                        const int32_t* perm, void* out, int T, int k, int E, int N, int K, int epilogue, void* stream) {
  return tiled_entry<MT_MX4>(rows_in, q_frag, s_frag, offs, perm, out, T, k, E, N, K, epilogue, stream);
}

extern "C" int ssd_moe_gemm_tiled_fp8b(const void* rows_in, const void* q_frag, const float* s_grp, const int32_t* offs,
                                       const int32_t* perm, void* out, int T, int k, int E, int N, int K, int epilogue, void* stream) {
  return tiled_entry<MT_FP8B>(rows_in, q_frag, s_grp, offs, perm, out, T, k, E, N, K, epilogue, stream);
}

// Guided decoding (include/ssd_hip_guide.h has the semantics): a token automaton per sequence in CSR tables, walked through the round's
// tokens by one wave per sequence (guide_walk_kernel), and the allow set of every row's state written over the raw logit rows
// (guide_rows_kernel, the shape of constrain_rows_kernel: workgroup (slice, row) owns 4096 entries, two 8-entry chunks per thread).
//
// Both kernels find edges with one primitive, a wave-wide lower bound over a state's sorted edge tokens: 64 lanes probe 64 evenly
// spaced edges, a ballot tells which stride holds the key, and the range shrinks by 64 per round -- two rounds take 262144 edges down
// to 64, which the lanes then compare one each.  A walked token costs the state's two offsets, its default, at most four dependent
// probe loads and the edge's next state, whatever the state's size; a per-lane binary search over 262144 edges would be 18 dependent
// loads.  Everything a wave decides comes out of ballots, so all its lanes hold the same range and the same state.
//
// The rows kernel builds the slice's 4096-bit allow bitmap in LDS: all ones under a default, all zeros without; the state's edges
// inside the slice (two lower bounds) then set their bit (next != -1) or clear it (next == -1) with LDS atomics.  OR and AND-NOT
// commute and a token has one edge at most, so the bits do not depend on the order.  Each thread then bans ~allow of its chunks with
// the write rules of constrain.hip (ban_chunk, rows.h): nothing banned -- neither read nor written; all banned -- one 16-byte store; otherwise 16-byte
// load, banned halves replaced, 16-byte store; a chunk that crosses V or an unaligned row -- 2-byte stores.  One writer per entry.
#include "common.h"
#include "rows.h"

constexpr int GD_THREADS = 256;
constexpr int GD_PER = 2;                                               // 8-entry chunks per thread
constexpr int GD_WORDS = SSD_GUIDE_SLICE / 32;
constexpr int GD_ROUNDS = 2;                                            // narrowing rounds of the search: 64^(GD_ROUNDS + 1) edges
static_assert(SSD_GUIDE_SLICE == GD_THREADS * GD_PER * 8, "one slice = two chunks per thread");
static_assert(GD_WORDS <= GD_THREADS, "one thread per bitmap word");
static_assert(SSD_GUIDE_MAX_EDGES == 64 * 64 * 64, "two narrowing rounds and a compare per lane");

// First index i in [a, b) with tok[i] >= key (b if there is none); tok sorted, strictly increasing.  Called by a whole wave with the
// same arguments in every lane; returns the same value in every lane.
__device__ __forceinline__ int wave_lower_bound(const int32_t* __restrict__ tok, int a, int b, int key, int lane) {
#pragma unroll
  for (int r = 0; r < GD_ROUNDS; ++r) {
    const int n = b - a;
    if (n <= 64) break;
    const int stride = (n + 63) >> 6;
    const long long p = (long long)a + (long long)lane * stride;
    const bool less = p < b && tok[p] < key;
    const int c = __popcll(__ballot(less));         // sorted: the lanes below c saw a smaller token
    if (c == 0) return a;
    const long long nb = (long long)a + (long long)c * stride;
    a = a + (c - 1) * stride + 1;
    b = nb < b ? (int)nb : b;
  }
  const int p = a + lane;
  const bool less = p < b && tok[p] < key;
  return a + __popcll(__ballot(less));
}

struct GuideState {         // what one state of sequence b's automaton needs: the edge range (empty if malformed) and the default
  int o0, o1, dflt;
};

__device__ __forceinline__ int gd_next(int nx, int ns) { return (nx >= 0 && nx < ns) ? nx : -1; }

__device__ __forceinline__ GuideState gd_state(const int32_t* __restrict__ edge_off, const int32_t* __restrict__ dflt, int b, int s, int ns,
                                               int states_ld, int edges_ld) {
  const int32_t* off = edge_off + (size_t)b * (states_ld + 1) + s;
  GuideState g;
  g.o0 = off[0];
  g.o1 = off[1];
  g.dflt = gd_next(dflt[(size_t)b * states_ld + s], ns);
  if (g.o0 < 0 || g.o1 > edges_ld || g.o1 < g.o0) g.o0 = g.o1 = 0;
  return g;
}

__global__ void __launch_bounds__(64)
guide_walk_kernel(int32_t* __restrict__ state_rows, int T, int rows_per_seq, const int32_t* __restrict__ guide_on,
                  const int32_t* __restrict__ state0, const int32_t* __restrict__ n_states, const int32_t* __restrict__ edge_off,
                  const int32_t* __restrict__ dflt, const int32_t* __restrict__ edge_tok, const int32_t* __restrict__ edge_next, int states_ld,
                  int edges_ld, const int64_t* __restrict__ extra, int extra_ld, const int32_t* __restrict__ extra_n) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int r0 = b * rows_per_seq;
  const int rows = min(rows_per_seq, T - r0);
  const int ns = min(max(n_states[b], 0), states_ld);
  int s = state0[b];
  if (guide_on[b] == 0 || s < 0 || s >= ns) s = -1;
  const bool prefix = extra && !extra_n;
  // steps the last row sees; the prefix form writes a row in front of every step (rows <= rows_per_seq <= extra_ld there)
  const int steps = prefix ? rows - 1 : rows_seen(extra, extra_ld, extra_n, r0, b, rows_per_seq);
  const int32_t* tok = edge_tok + (size_t)b * edges_ld;
  const int32_t* nxt = edge_next + (size_t)b * edges_ld;
  for (int k = 0; k < steps; ++k) {           // (bounded by extra_ld - 1 <= SSD_GUIDE_MAX_EXTRA)
    if (prefix && lane == 0) state_rows[r0 + k] = s;
    if (s < 0) continue;                      // -1 stays -1; the prefix form still has rows to write
    const long long t = extra[(size_t)b * extra_ld + 1 + k];
    if (t < 0 || t > 0x7fffffffll) {
      s = -1;
      continue;
    }
    const GuideState g = gd_state(edge_off, dflt, b, s, ns, states_ld, edges_ld);
    const int i = wave_lower_bound(tok, g.o0, g.o1, (int)t, lane);
    s = (i < g.o1 && tok[i] == (int)t) ? gd_next(nxt[i], ns) : g.dflt;
  }
  if (prefix) {
    if (lane == 0) state_rows[r0 + rows - 1] = s;
  } else {
    for (int j = lane; j < rows; j += 64) state_rows[r0 + j] = s;
  }
}

__global__ void __launch_bounds__(GD_THREADS)
guide_rows_kernel(bf16_t* __restrict__ logits, long ld, int V, const int32_t* __restrict__ state_rows, int rows_per_seq,
                  const int32_t* __restrict__ n_states, const int32_t* __restrict__ edge_off, const int32_t* __restrict__ dflt,
                  const int32_t* __restrict__ edge_tok, const int32_t* __restrict__ edge_next, int states_ld, int edges_ld) {
  __shared__ uint32_t allow[GD_WORDS];
  const int row = blockIdx.y, sl = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int b = row / rows_per_seq;
  const int s = state_rows[row];
  const int ns = min(max(n_states[b], 0), states_ld);
  if (s < 0 || s >= ns) return;                 // no guide in front of this row (uniform over the workgroup)
  const GuideState g = gd_state(edge_off, dflt, b, s, ns, states_ld, edges_ld);
  const int lo = sl * SSD_GUIDE_SLICE, hi = min(lo + SSD_GUIDE_SLICE, V);
  const int32_t* tok = edge_tok + (size_t)b * edges_ld;
  const int32_t* nxt = edge_next + (size_t)b * edges_ld;
  // the state's edges inside [lo, hi): every wave searches for itself (the same few loads, no barrier in front of the early exit)
  const int e0 = wave_lower_bound(tok, g.o0, g.o1, lo, lane);
  const int e1 = wave_lower_bound(tok, e0, g.o1, hi, lane);
  const bool open = g.dflt >= 0;
  if (open && e0 == e1) return;                 // a default and no exception in this slice: nothing is banned (uniform)
  if (tid < GD_WORDS) allow[tid] = open ? 0xffffffffu : 0u;
  __syncthreads();
#pragma unroll 1
  for (int k = 0; k < SSD_GUIDE_SLICE / GD_THREADS; ++k) {          // sorted and strictly increasing: at most one edge per entry
    const int i = e0 + k * GD_THREADS + tid;
    if (i < e1) {
      const int d = tok[i] - lo;
      if (d >= 0 && d < hi - lo) {
        if (gd_next(nxt[i], ns) >= 0) atomicOr(&allow[d >> 5], 1u << (d & 31));
        else atomicAnd(&allow[d >> 5], ~(1u << (d & 31)));
      }
    }
  }
  __syncthreads();

  bf16_t* x = logits + (size_t)row * ld;
  const bool vec = (reinterpret_cast<uintptr_t>(x) & 15) == 0;
#pragma unroll
  for (int u = 0; u < GD_PER; ++u) {
    const int c = u * GD_THREADS + tid;         // chunk of the slice
    const int base = lo + c * 8;
    if (base >= V) continue;
    uint32_t ban = ~(allow[c >> 2] >> ((c & 3) * 8)) & 0xffu;
    ban_chunk(x, base, V, vec, ban);
  }
}

static int guide_tables_check(const int32_t* n_states, const int32_t* edge_off, const int32_t* dflt, const int32_t* edge_tok,
                              const int32_t* edge_next, int states_ld, int edges_ld) {
  if (states_ld < 1 || edges_ld < 1 || edges_ld > SSD_GUIDE_MAX_EDGES) return SSD_ERR_SHAPE;
  if (!n_states || !edge_off || !dflt || !edge_tok || !edge_next) return SSD_ERR_ARG;
  return SSD_OK;
}

extern "C" int ssd_guide_walk(int32_t* state_rows, int T, int rows_per_seq, const int32_t* guide_on, const int32_t* state0,
                              const int32_t* n_states, const int32_t* edge_off, const int32_t* dflt, const int32_t* edge_tok,
                              const int32_t* edge_next, int states_ld, int edges_ld, const int64_t* extra, int extra_ld,
                              const int32_t* extra_n, void* stream) {
  if (T <= 0 || rows_per_seq <= 0 || T > 65535) return SSD_ERR_SHAPE;
  if (extra && (extra_ld < 1 || extra_ld - 1 > SSD_GUIDE_MAX_EXTRA || (!extra_n && extra_ld < rows_per_seq))) return SSD_ERR_SHAPE;
  const int rc = guide_tables_check(n_states, edge_off, dflt, edge_tok, edge_next, states_ld, edges_ld);
  if (rc == SSD_ERR_SHAPE) return rc;
  if (!state_rows || !guide_on || !state0 || rc != SSD_OK || (extra_n && !extra)) return SSD_ERR_ARG;
  const int B = (T + rows_per_seq - 1) / rows_per_seq;
  hipLaunchKernelGGL(guide_walk_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, state_rows, T, rows_per_seq, guide_on, state0, n_states,
                     edge_off, dflt, edge_tok, edge_next, states_ld, edges_ld, extra, extra_ld, extra_n);
  return hipGetLastError() == hipSuccess ? SSD_OK : SSD_ERR_LAUNCH;
}

extern "C" int ssd_guide_rows(void* logits_rows, long ld, int T, int V, const int32_t* state_rows, int rows_per_seq,
                              const int32_t* n_states, const int32_t* edge_off, const int32_t* dflt, const int32_t* edge_tok,
                              const int32_t* edge_next, int states_ld, int edges_ld, void* stream) {
  if (T <= 0 || V <= 0 || rows_per_seq <= 0 || ld < V || T > 65535) return SSD_ERR_SHAPE;
  const int rc = guide_tables_check(n_states, edge_off, dflt, edge_tok, edge_next, states_ld, edges_ld);
  if (rc == SSD_ERR_SHAPE) return rc;
  if (!logits_rows || !state_rows || rc != SSD_OK) return SSD_ERR_ARG;
  const int S = (V + SSD_GUIDE_SLICE - 1) / SSD_GUIDE_SLICE;
  hipLaunchKernelGGL(guide_rows_kernel, dim3(S, T), dim3(GD_THREADS), 0, (hipStream_t)stream, (bf16_t*)logits_rows, ld, V, state_rows,
                     rows_per_seq, n_states, edge_off, dflt, edge_tok, edge_next, states_ld, edges_ld);
  return hipGetLastError() == hipSuccess ? SSD_OK : SSD_ERR_LAUNCH;
}

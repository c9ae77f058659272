/*
 * libssdhip -- guided decoding: a deterministic automaton over token ids per sequence, walked on the device through the round's
 * tokens, and its allow set written over raw logit rows, in place, beside ssd_penalize_rows and ssd_constrain_rows and in front of
 * the temperature, ssd_filter_rows, the samplers, ssd_row_lse, ssd_verify_ratio and argmax.
 *
 * Additive to ssd_hip.h (same conventions, error codes and ABI version).  This comment is the normative text.
 *
 * THE AUTOMATON of batch row b has the states 0 .. n_states[b] - 1 and lives in five tables with one slot per batch row:
 *   n_states  int32 [B]                     number of states (clamped to [0, states_ld])
 *   edge_off  int32 [B][states_ld + 1]      CSR offsets: the edges of state s are e in [edge_off[b][s], edge_off[b][s + 1])
 *   dflt      int32 [B][states_ld]          default next state of each state
 *   edge_tok  int32 [B][edges_ld]           the token of edge e; the edges of one state are sorted by token, strictly increasing
 *   edge_next int32 [B][edges_ld]           the next state of edge e
 * A next state (of an edge or a default) outside [-1, n_states[b]) reads as -1.  A state whose offsets leave [0, edges_ld] or run
 * backwards has no edges.  With that,
 *   delta(s, t) = the next state of the edge (s, t) if state s has an edge on token t, otherwise dflt[b][s];   delta(-1, t) = -1
 * and token t is ALLOWED at state s if and only if delta(s, t) != -1.  So a state without a default allows exactly the tokens of its
 * edges whose next state is not -1, and a state with a default allows everything but the tokens of its edges whose next state is -1
 * (an edge to -1 is an explicit ban: the exception form).  State -1 means "no guide": nothing is banned there.
 *
 * ssd_guide_walk writes state_rows, int32 [T]: the state in front of every row (the row predicts the token that follows it).
 * rows_per_seq consecutive rows belong to one sequence b = row / rows_per_seq (1 for decode rows, K + 1 for verify rows).  A row's
 * state is state0[b] -- the host's state in front of the sequence's first row of the round, the token fed to that row included --
 * advanced by delta through the extras the row sees, which are exactly the buffer and the two forms of ssd_penalize_rows and
 * ssd_constrain_rows:
 *   extra[b][0 .. extra_ld)         int64; entry 0 is the token fed to the first row (state0 has consumed it already) and
 *     prefix form (extra_n == NULL)   row j of sequence b (j = row % rows_per_seq) sees extra[b][1 .. j]; row 0 sees none
 *     chain form  (extra_n != NULL)   every row of sequence b sees extra[b][1 .. n], n = min(max(*extra_n, 0), extra_ld - 1)
 *   Without extra every row's state is the start value.  The start value is -1 if guide_on[b] == 0 or state0[b] is outside
 *   [0, n_states[b]); a negative extra (or one past 2^31 - 1) gives -1; -1 stays -1.  All values are integers: the result is exact.
 *
 * ssd_guide_rows takes logits_rows, bf16 [T][ld], and state_rows.  Entry t in [0, V) of a row whose state s is in [0, n_states[b])
 * becomes -inf (bits 0xFF80) if t is not allowed at s, whatever it held, a NaN included.  Every other entry keeps its bits: allowed
 * entries (NaNs too), all of [V, ld), and every row whose state is -1 or outside [0, n_states[b]).  Edge tokens outside [0, V) ban and
 * allow nothing.  Nothing guards a row whose every entry ends up banned (a state without edges and without a default, or the
 * composition with the other constraints): that is the caller's error, as in ssd_hip_constrain.h.
 *
 * All per-round values -- tables, guide_on, state0, extras, *extra_n, state_rows -- are read from device memory when the kernels
 * run, so a captured graph replays with fresh data.  Neither call allocates, synchronises or uses global atomics.  The walk runs one
 * wave per sequence and finds an edge with a wave-wide search (64 probes, ballot, narrow: two such rounds, then one compare per
 * lane), so a step costs a few dependent loads whatever the state's size; every loop is bounded by a constant, by extra_ld or by
 * rows_per_seq.  The rows kernel builds each 4096-entry slice's allow bitmap in LDS with integer OR / AND-NOT (they commute, and a
 * token has at most one edge per state) and every entry has exactly one writing thread: the same input gives the same bits on every
 * run, inside and outside a hipGraph.  -inf stays -inf under ssd_penalize_rows and ssd_constrain_rows, so the order of the three
 * calls does not matter.
 */
#ifndef SSD_HIP_GUIDE_H
#define SSD_HIP_GUIDE_H
#include "ssd_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Most states and edges of one automaton the host accepts (the strides of the engine's tables); the calls take any strides >= 1,
 * edges_ld up to SSD_GUIDE_MAX_EDGES = 64^3: what two narrowing rounds of 64 and one compare per lane can search. */
#define SSD_GUIDE_MAX_STATES 16384
#define SSD_GUIDE_MAX_EDGES 262144
/* Most extra tokens one row can see (extra_ld - 1); the bound of SSD_PENALTY_MAX_EXTRA and SSD_CONSTRAIN_MAX_EXTRA. */
#define SSD_GUIDE_MAX_EXTRA 64
/* Entries of a row one workgroup handles (grid: slices x rows). */
#define SSD_GUIDE_SLICE 4096

/* The tables (n_states, edge_off, dflt, edge_tok, edge_next with states_ld and edges_ld) are one group and are required whole; the
 * extras (extra with extra_ld and, for the chain form, extra_n) are optional.
 * SSD_ERR_SHAPE for T or rows_per_seq <= 0, T > 65535, states_ld < 1, edges_ld < 1 or > SSD_GUIDE_MAX_EDGES, extra with
 * extra_ld < 1 or extra_ld - 1 > SSD_GUIDE_MAX_EXTRA, or the prefix form with extra_ld < rows_per_seq; SSD_ERR_ARG for a null
 * state_rows, guide_on or state0, a table given in part (any of the five null), or extra_n without extra. */
int ssd_guide_walk(int32_t* state_rows, int T, int rows_per_seq, const int32_t* guide_on, const int32_t* state0, const int32_t* n_states,
                   const int32_t* edge_off, const int32_t* dflt, const int32_t* edge_tok, const int32_t* edge_next, int states_ld,
                   int edges_ld, const int64_t* extra, int extra_ld, const int32_t* extra_n, void* stream);

/* SSD_ERR_SHAPE for T, V or rows_per_seq <= 0, T > 65535, ld < V, states_ld < 1, edges_ld < 1 or > SSD_GUIDE_MAX_EDGES;
 * SSD_ERR_ARG for a null logits_rows or state_rows or a table given in part. */
int ssd_guide_rows(void* logits_rows, long ld, int T, int V, const int32_t* state_rows, int rows_per_seq, const int32_t* n_states,
                   const int32_t* edge_off, const int32_t* dflt, const int32_t* edge_tok, const int32_t* edge_next, int states_ld,
                   int edges_ld, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SSD_HIP_GUIDE_H */

"""ssd_logprob_rows_known (csrc/prompt_logprob.hip) on the GPU: lse, the top list and the token's log-probability equal BY BITS to what
ssd_logprob_rows + ssd_logprob_pick (csrc/logprob.hip) leave for the same rows, whatever the rows' alignment, and the rank equal to the
float64 restatement in tests/prompt_logprob_ref.py (a count of integers: exact).  Rows are bf16 normal deviates, which tie often, with
+inf / NaN sentinels behind every row where ld > V; every output buffer is sentinel-filled beforehand, and the token of a skipped row is
a poisoned index that must not be read.  T <= 6 everywhere; the two large vocabularies run T = 2."""
import ctypes

import numpy as np
import pytest
import torch

from tests import prompt_logprob_ref as PR
from tests.test_hip_logprob import BF, MAXN, S_ID, S_LSE, S_OUT, S_VAL, TOL, bits, close, with_sentinels

pytestmark = pytest.mark.gpu

S_RANK = -4242
POISON = 1 << 40            # tokens[t] of a skipped row: as an index it is far outside any allocation


@pytest.fixture(scope="module")
def P():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ssd_amd.hip import prompt_logprob_ops
    return prompt_logprob_ops


@pytest.fixture(scope="module")
def L(P):
    from ssd_amd.hip import logprob_ops
    return logprob_ops


def normal_rows(T: int, V: int, seed: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(T, V, generator=g) * 3).to(BF)


class Out:
    pass


def device_rows(rows: torch.Tensor, offset: int) -> torch.Tensor:
    """rows on the device, the first one `offset` entries behind a 256-byte boundary."""
    T, ld = rows.shape
    d = torch.zeros(T * ld + 16, dtype=BF, device="cuda")[offset:offset + T * ld].view(T, ld)
    d.copy_(rows)
    return d


def fresh_outputs(o, T: int):
    o.d_lse = torch.full((T,), S_LSE, dtype=torch.float32, device="cuda")
    o.d_val = torch.full((T, MAXN), S_VAL, dtype=torch.float32, device="cuda")
    o.d_id = torch.full((T, MAXN), S_ID, dtype=torch.int32, device="cuda")
    o.d_out = torch.full((T,), S_OUT, dtype=torch.float32, device="cuda")
    o.d_rank = torch.full((T,), S_RANK, dtype=torch.int32, device="cuda")


def read_back(o):
    torch.cuda.synchronize()
    o.lse, o.val, o.id = o.d_lse.cpu().numpy(), o.d_val.cpu().numpy(), o.d_id.cpu().numpy()
    o.out, o.rank = o.d_out.cpu().numpy(), o.d_rank.cpu().numpy()
    return o


def known(P, rows: torch.Tensor, V: int, n_tops, tokens, offset: int = 0, top: bool = True):
    T, ld = rows.shape
    o = Out()
    o.d_rows = device_rows(rows, offset)
    o.d_ntop = torch.tensor(list(n_tops), dtype=torch.int32, device="cuda")
    o.d_tok = torch.tensor(list(tokens), dtype=torch.int64, device="cuda")
    fresh_outputs(o, T)
    o.d_ws = torch.zeros(P.logprob_known_ws_bytes(T, V) // 4, dtype=torch.float32, device="cuda")
    P.logprob_rows_known(o.d_rows, ld, T, V, o.d_ntop, o.d_tok, o.d_lse, o.d_val if top else None, o.d_id if top else None, o.d_out,
                         o.d_rank, o.d_ws)
    read_back(o)
    assert np.array_equal(bits(o.d_rows.cpu()), bits(rows)), "the rows are read only"
    return o


def pair(L, rows: torch.Tensor, V: int, n_tops, tokens, offset: int = 0):
    """The existing launches on the same rows: ssd_logprob_rows, then ssd_logprob_pick on the live rows (a skipped row's token is not
    poisoned here: the pick reads it)."""
    T, ld = rows.shape
    o = Out()
    o.d_rows = device_rows(rows, offset)
    o.d_ntop = torch.tensor(list(n_tops), dtype=torch.int32, device="cuda")
    o.d_tok = torch.tensor([0 if t == POISON else t for t in tokens], dtype=torch.int64, device="cuda")
    fresh_outputs(o, T)
    o.d_ws = torch.zeros(L.logprob_rows_ws_bytes(T, V) // 4, dtype=torch.float32, device="cuda")
    L.logprob_rows(o.d_rows, ld, T, V, o.d_ntop, 1, o.d_lse, o.d_val, o.d_id, o.d_ws)
    L.logprob_pick(o.d_rows, ld, T, V, o.d_tok, o.d_lse, o.d_ntop, 1, o.d_out)
    return read_back(o)


def i32(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a).view(np.int32)


def same_bits(a, b, what: str, rank: bool = True):
    for f in ("lse", "val", "out"):
        assert np.array_equal(i32(getattr(a, f)), i32(getattr(b, f))), f"{what}: {f} differs by bits"
    assert np.array_equal(a.id, b.id), f"{what}: top ids differ"
    if rank:
        assert np.array_equal(a.rank, b.rank), f"{what}: ranks differ"


def check(rows: torch.Tensor, o, V: int, n_tops, tokens, what: str):
    """Every per-row assertion that needs no second launch: skips, the rank and lse against the reference, the invariant."""
    x = rows[:, :V].to(torch.float64).numpy()
    for t in range(rows.shape[0]):
        n, tok = n_tops[t], tokens[t]
        w = f"{what} row {t} n_top {n} token {tok}"
        if n < 0 or n > MAXN:
            assert o.lse[t] == np.float32(S_LSE) and o.out[t] == np.float32(S_OUT) and o.rank[t] == S_RANK, f"{w}: written"
            assert (o.val[t] == np.float32(S_VAL)).all() and (o.id[t] == S_ID).all(), f"{w}: written"
            continue
        ref = PR.known_row(x[t], tok, n)
        assert int(o.rank[t]) == ref.rank, f"{w}: rank {o.rank[t]} vs {ref.rank}"
        assert close(float(o.lse[t]), ref.row.lse) <= TOL, f"{w}: lse {o.lse[t]} vs {ref.row.lse}"
        assert o.id[t, :n].tolist() == ref.row.top_id, f"{w}: top ids"
        assert (o.val[t, n:] == np.float32(S_VAL)).all() and (o.id[t, n:] == S_ID).all(), f"{w}: slots past n_top were written"
        if not 0 <= tok < V:
            assert np.isnan(o.out[t]) and o.rank[t] == 0, w
        elif not np.isinf(ref.row.lse):
            assert close(float(o.out[t]), ref.logprob) <= TOL, f"{w}: logprob {o.out[t]} vs {ref.logprob}"
        r = int(o.rank[t])
        if 1 <= r <= n:     # the token is among the r best: the r-th best has its value, so its log-probability by bits
            assert i32(o.val[t, r - 1:r])[0] == i32(o.out[t:t + 1])[0], f"{w}: top_val[rank - 1] is not out by bits"
            assert tok in o.id[t, :r].tolist(), f"{w}: the token is not among top_id[:rank]"


N_CYCLE = [5, 0, 20, 1, -1, 3]


def slice_tokens(V: int, T: int, seed: int) -> list:
    """One token per row, walking the 4096-entry slices (the ragged last one included) at varying offsets; the last row takes V - 1."""
    S = (V + 4095) // 4096
    g = np.random.default_rng(seed)
    toks = []
    for t in range(T):
        sl = t % S
        lo, hi = sl * 4096, min(V, (sl + 1) * 4096)
        toks.append(int(g.integers(lo, hi)))
    toks[-1] = V - 1
    return toks


@pytest.mark.parametrize("V", [1, 7, 4096, 4097, 8200, 12296])
def test_shapes_bits_against_rows_and_pick_in_every_alignment(P, L, V):
    T = 6
    x = normal_rows(T, V, 900 + V)
    tokens = slice_tokens(V, T, V)
    tokens[4] = POISON                                  # N_CYCLE[4] = -1: the row is skipped and its token never read
    ld8 = (V + 1 + 7) // 8 * 8
    layouts = [("ld = V", x, 0), ("ld = V + 1", with_sentinels(x, V + 1), 0),
               ("aligned", with_sentinels(x, ld8), 0), ("offset 1", with_sentinels(x, ld8), 1)]
    first = None
    for name, rows, offset in layouts:
        o = known(P, rows, V, N_CYCLE, tokens, offset)
        check(rows, o, V, N_CYCLE, tokens, f"V={V} {name}")
        same_bits(o, pair(L, rows, V, N_CYCLE, tokens, offset), f"V={V} {name}: known vs rows + pick", rank=False)
        if first is None:
            first = o
        same_bits(first, o, f"V={V}: {name} vs {layouts[0][0]}")


def test_rank_edges(P, L):
    V = 8200                                            # three slices, the last one ragged (8 entries)
    nan, inf = float("nan"), float("inf")
    a = normal_rows(6, V, 11)
    tok_a = [0] * 6
    a[0, 4094:4098] = 1.25; tok_a[0] = 4095             # a tie that straddles the border of slices 0 and 1, token on the left ...
    a[1, 8190:8194] = 0.75; tok_a[1] = 8192             # ... and one over the border to the ragged slice, token on the right
    crest = [3, 4095, 4096, 8191, 8199]
    a[2, crest] = 40.0; tok_a[2] = 8199                 # the maximum, 5-fold, in all three slices: rank 5
    a[3, 77] = 41.0; tok_a[3] = 77                      # a unique maximum: rank 1
    a[4, crest[:2]] = 40.0; tok_a[4] = 3                # two tied maxima: both rank 2
    a[5, 100:5000] = -inf; a[5, 5000:5010] = nan; tok_a[5] = 4200       # a -inf token: every comparable entry counts
    n_a = [5, 3, 20, 1, 1, 0]
    b = normal_rows(6, V, 12)
    tok_b = [0] * 6
    b[0] = -(b[0].abs()); b[0, 0:6000:3] = 0.0; b[0, 1:6000:3] = -0.0; tok_b[0] = 4                # a -0.0 token: +0.0 entries count
    b[1] = b[0]; tok_b[1] = 3                           # ... and a +0.0 token: -0.0 entries count
    b[2, 10:20] = nan; b[2, 4096] = nan; tok_b[2] = 4096                # a NaN token entry: NaN, rank 0
    tok_b[3], tok_b[4] = -1, V                          # tokens outside [0, V): NaN, rank 0
    b[5, :] = nan; b[5, 8199] = -2.0; tok_b[5] = 8199   # one comparable entry, in the ragged slice: rank 1
    n_b = [20, 20, 5, 2, 0, 4]
    for x, toks, n_tops, what in ((a, tok_a, n_a, "a"), (b, tok_b, n_b, "b")):
        rows = with_sentinels(x, V + 4)                 # +inf / NaN in [V, ld): never counted
        o = known(P, rows, V, n_tops, toks)
        check(rows, o, V, n_tops, toks, f"edges {what}")
        same_bits(o, pair(L, rows, V, n_tops, toks), f"edges {what}: known vs rows + pick", rank=False)
        same_bits(o, known(P, rows, V, n_tops, toks, offset=1), f"edges {what}: aligned vs offset 1")
        if what == "a":
            assert o.rank[:5].tolist() == [int((x[0, :V].double() >= 1.25).sum()), int((x[1, :V].double() >= 0.75).sum()), 5, 1, 2]
            assert o.rank[5] == V - 10
        else:
            assert o.rank[0] == o.rank[1] == 4000 and o.rank[2:].tolist() == [0, 0, 0, 1]        # (2000 of each zero)
            assert np.isnan(o.out[2:5]).all() and o.out[5] == 0.0


def test_skips_and_rows_without_a_top_list(P, L):
    V = 4100
    x = normal_rows(6, V, 21)
    rows = with_sentinels(x, V + 4)
    n_tops = [-1, 0, 21, 0, -7, 2]                      # 21 and -7 are skips like -1
    toks = [POISON, 5, POISON, 4099, -POISON, 4097]
    o = known(P, rows, V, n_tops, toks)
    check(rows, o, V, n_tops, toks, "skips")
    for t in (1, 3):                                    # n_top = 0: lse, out and rank only
        assert (o.val[t] == np.float32(S_VAL)).all() and (o.id[t] == S_ID).all() and o.rank[t] >= 1 and o.out[t] < 0
    # without top_val / top_id: the same lse, out and rank
    q = known(P, rows, V, n_tops, toks, top=False)
    assert (q.val == np.float32(S_VAL)).all() and (q.id == S_ID).all()
    for f in ("lse", "out", "rank"):
        assert np.array_equal(i32(getattr(o, f)), i32(getattr(q, f))), f


@pytest.fixture(scope="module")
def large(P):
    out = {}
    for V in (128256, 196608):
        x = normal_rows(2, V, V)
        x[1] = (x[1].float() * 2).round().to(BF) / 2    # a handful of values: ties in every slice
        rows = with_sentinels(x, V + 8)
        n_tops, toks = [20, 5], [V - 1, 4096 * 7 + 1]
        out[V] = (rows, n_tops, toks, known(P, rows, V, n_tops, toks))
    return out


@pytest.mark.parametrize("V", [128256, 196608])
def test_real_vocabularies(P, L, large, V):
    rows, n_tops, toks, o = large[V]
    check(rows, o, V, n_tops, toks, f"V={V}")
    same_bits(o, pair(L, rows, V, n_tops, toks), f"V={V}: known vs rows + pick", rank=False)
    same_bits(o, known(P, rows, V, n_tops, toks, offset=1), f"V={V}: aligned vs offset 1")
    assert o.rank[1] > 1000                             # (the quantised row's token does sit under a crowd of ties and larger values)


def test_two_runs_and_a_graph_replay_are_bit_equal(P, large):
    from ssd_amd.utils.graphs import capture
    V = 128256
    rows, n_tops, toks, a = large[V]
    ld = rows.shape[1]
    o = known(P, rows, V, n_tops, toks)
    same_bits(a, o, "second run")
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with capture(graph, stream=stream):
        P.logprob_rows_known(o.d_rows, ld, 2, V, o.d_ntop, o.d_tok, o.d_lse, o.d_val, o.d_id, o.d_out, o.d_rank, o.d_ws)

    def refill():
        o.d_lse.fill_(S_LSE); o.d_val.fill_(S_VAL); o.d_id.fill_(S_ID); o.d_out.fill_(S_OUT); o.d_rank.fill_(S_RANK)

    refill()
    graph.replay()
    same_bits(a, read_back(o), "replay")
    # other tokens and counts on the device, no new capture: the replay follows them
    n2, t2 = [-1, 20], [POISON, 5]
    o.d_ntop.copy_(torch.tensor(n2, dtype=torch.int32))
    o.d_tok.copy_(torch.tensor(t2, dtype=torch.int64))
    refill()
    graph.replay()
    check(rows, read_back(o), V, n2, t2, "replay with fresh tokens and n_top")
    same_bits(o, known(P, rows, V, n2, t2), "replay with fresh inputs vs an eager run")


def test_refusals(P):
    """Every refusal of the header returns its code; none reaches a launch (the outputs keep their sentinels)."""
    lib = P.load_prompt_logprob_library()
    SHAPE, ARG = -1, -3                                 # SSD_ERR_SHAPE, SSD_ERR_ARG (include/ssd_hip.h)
    o = Out()
    fresh_outputs(o, 2)
    z = torch.zeros(64, dtype=BF, device="cuda")
    nt = torch.zeros(2, dtype=torch.int32, device="cuda")
    tk = torch.zeros(2, dtype=torch.int64, device="cuda")
    ws = torch.zeros(P.logprob_known_ws_bytes(2, 32) // 4, dtype=torch.float32, device="cuda")
    base = dict(rows=z, ld=32, T=2, V=32, n_top=nt, tokens=tk, lse=o.d_lse, val=o.d_val, id=o.d_id, out=o.d_out, rank=o.d_rank, ws=ws)

    def call(**kw):
        a = dict(base, **kw)
        p = lambda t: ctypes.c_void_p(None if t is None else t.data_ptr())
        return lib.ssd_logprob_rows_known(p(a["rows"]), a["ld"], a["T"], a["V"], p(a["n_top"]), p(a["tokens"]), p(a["lse"]), p(a["val"]),
                                          p(a["id"]), p(a["out"]), p(a["rank"]), p(a["ws"]), None)

    for kw in (dict(T=0), dict(T=-1), dict(V=0), dict(V=-3), dict(T=65536), dict(ld=31), dict(V=P.MAX_V + 1, ld=P.MAX_V + 1)):
        assert call(**kw) == SHAPE, kw
    for name in ("rows", "n_top", "tokens", "lse", "out", "rank", "ws", "val", "id"):
        assert call(**{name: None}) == ARG, name
    for T, V in ((0, 32), (2, 0), (2, P.MAX_V + 1)):
        assert lib.ssd_logprob_known_ws_bytes(T, V) == SHAPE
    assert lib.ssd_logprob_known_ws_bytes(3, 4097) == 3 * 2 * 44 * 4
    read_back(o)
    assert (o.lse == np.float32(S_LSE)).all() and (o.out == np.float32(S_OUT)).all() and (o.rank == S_RANK).all()
    assert (o.val == np.float32(S_VAL)).all() and (o.id == S_ID).all()
    assert call() == 0 and call(val=None, id=None) == 0       # (the same arguments, untouched, do launch)
    torch.cuda.synchronize()

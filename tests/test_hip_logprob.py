"""ssd_logprob_rows / ssd_logprob_pick / ssd_logprob_pick_verify (csrc/logprob.hip) on the GPU against the float64 restatement in
tests/logprob_ref.py, in a few launches: vocabulary sizes around the 8-entry chunk, SSD_LOGPROB_MAX_N and the 4096-entry slice, the two
real ones (128256, 151936), n_top in {-1, 0, 1, 5, 20} mixed within one launch through rows_per_param in {1, 4}, ld > V with +inf / NaN
sentinels behind every row, aligned rows (16-byte loads) and rows offset by an odd number of entries (2-byte loads), and every output
buffer sentinel-filled beforehand: skipped rows, slots past n_top and copy entries past V must come back untouched.

top_id must equal the reference's exactly (bf16 values compare exactly; ties by lowest index, also across slice borders: rows
quantised to a handful of values at V = 128256).  lse and every log-probability: within TOL = 2e-3 absolute of the float64 reference,
the cap tests/test_hip_sample_edges.py gives ssd_row_lse, with logits in +-30 (fp32 sums of 16 terms per thread, 256 partials per
slice, at most 48 slices, __expf).  Measured on one MI355X: see DESIGN.md, "Log-probabilities".  The copy equals the input by bits."""
import numpy as np
import pytest
import torch

from tests import logprob_ref as R

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
TOL = 2e-3
MAXN = R.MAX_N
S_LSE, S_VAL, S_ID, S_OUT, S_RAW = -777.0, -555.0, -9, -333.0, 0x1234       # what every output buffer holds before a launch
WORST = {"lse": 0.0, "top": 0.0, "pick": 0.0}


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ssd_amd.hip import logprob_ops
    return logprob_ops


def bits(t: torch.Tensor) -> np.ndarray:
    return t.contiguous().view(torch.int16).cpu().numpy().astype(np.int64) & 0xFFFF


def with_sentinels(x: torch.Tensor, ld: int) -> torch.Tensor:
    """[T, V] -> [T, ld] with +inf and NaN behind every row."""
    T, V = x.shape
    out = torch.empty(T, ld, dtype=BF)
    out[:, :V] = x
    out[:, V:] = torch.tensor([float("inf"), float("nan")], dtype=BF).repeat((ld - V + 1) // 2)[:ld - V]
    return out


def random_rows(T: int, V: int, seed: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(T, V, generator=g) - 0.5) * 60).to(BF)


class Out:
    pass


def launch(L, rows: torch.Tensor, V: int, n_tops, rpp: int, offset: int = 0, copy: bool = True, raw_pad: int = 5, raw_offset: int = 0):
    """rows bf16 [T, ld] on the host -> the outputs on the host (and the device tensors, for the picks).  offset: the first row
    starts that many entries behind a 16-byte boundary (an odd offset with an even ld: no row can take the 16-byte loads)."""
    T, ld = rows.shape
    o = Out()
    o.d_rows = torch.zeros(T * ld + 8, dtype=BF, device="cuda")[offset:offset + T * ld].view(T, ld)
    o.d_rows.copy_(rows)
    o.d_ntop = torch.tensor(list(n_tops), dtype=torch.int32, device="cuda")
    o.d_lse = torch.full((T,), S_LSE, dtype=torch.float32, device="cuda")
    o.d_val = torch.full((T, MAXN), S_VAL, dtype=torch.float32, device="cuda")
    o.d_id = torch.full((T, MAXN), S_ID, dtype=torch.int32, device="cuda")
    o.raw_ld = V + raw_pad
    o.d_raw = None
    if copy:
        o.d_raw = torch.full((T * o.raw_ld + 8,), S_RAW, dtype=torch.int16, device="cuda").view(BF)[raw_offset:raw_offset + T * o.raw_ld]
        o.d_raw = o.d_raw.view(T, o.raw_ld)
    o.d_ws = torch.zeros(L.logprob_rows_ws_bytes(T, V) // 4, dtype=torch.float32, device="cuda")
    L.logprob_rows(o.d_rows, ld, T, V, o.d_ntop, rpp, o.d_lse, o.d_val, o.d_id, o.d_ws, raw_copy=o.d_raw, raw_ld=o.raw_ld if copy else 0)
    torch.cuda.synchronize()
    assert np.array_equal(bits(o.d_rows.cpu()), bits(rows)), "the rows are read only"
    o.lse, o.val, o.id = o.d_lse.cpu().numpy(), o.d_val.cpu().numpy(), o.d_id.cpu().numpy()
    o.raw = bits(o.d_raw.cpu()) if copy else None
    return o


def close(got: float, want: float) -> float:
    """|got - want| with equal infinities and NaN pairs counting as 0."""
    if np.isnan(want) or np.isnan(got):
        assert np.isnan(want) and np.isnan(got), (got, want)
        return 0.0
    if np.isinf(want) or np.isinf(got):
        assert got == want, (got, want)
        return 0.0
    return abs(got - want)


def check_launch(rows: torch.Tensor, o, V: int, n_tops, rpp: int, what: str):
    """All per-row assertions of one launch; returns the references of its rows (None for skipped ones)."""
    x = rows[:, :V].to(torch.float64).numpy()
    inb = bits(rows)
    refs = []
    for t in range(rows.shape[0]):
        n = n_tops[t // rpp]
        w = f"{what} row {t} n_top {n}"
        if n < 0:
            assert o.lse[t] == np.float32(S_LSE) and (o.val[t] == np.float32(S_VAL)).all() and (o.id[t] == S_ID).all(), f"{w}: written"
            if o.raw is not None:
                assert (o.raw[t] == S_RAW).all(), f"{w}: the copy of a skipped row was written"
            refs.append(None)
            continue
        ref = R.logprob_row(x[t], n)
        refs.append(ref)
        WORST["lse"] = max(WORST["lse"], close(float(o.lse[t]), ref.lse))
        assert close(float(o.lse[t]), ref.lse) <= TOL, f"{w}: lse {o.lse[t]} vs {ref.lse}"
        assert o.id[t, :n].tolist() == ref.top_id, f"{w}: top ids {o.id[t, :n].tolist()} vs {ref.top_id}"
        for f in range(n):
            d = close(float(o.val[t, f]), ref.top_val[f])
            WORST["top"] = max(WORST["top"], d)
            assert d <= TOL, f"{w}: top value {f}: {o.val[t, f]} vs {ref.top_val[f]}"
        assert (o.val[t, n:] == np.float32(S_VAL)).all() and (o.id[t, n:] == S_ID).all(), f"{w}: slots past n_top were written"
        if o.raw is not None:
            assert np.array_equal(o.raw[t, :V], inb[t, :V]), f"{w}: the copy differs from the row"
            assert (o.raw[t, V:] == S_RAW).all(), f"{w}: copy entries past V were written"
    return refs


N_CYCLE = [5, -1, 0, 1, 20, 20, 5, -1, 1, 0]


@pytest.mark.parametrize("V", [1, 7, 8, 20, 21, 1000, 1024, 1025, 4095, 4096, 4097, 8200])
def test_small_vocabularies_aligned_and_unaligned(L, V):
    T = 10
    x = random_rows(T, V, 100 + V)
    x[3, :] = x[3, 0]                                   # one row of V equal values: the top list is 0, 1, 2, ...
    if V > 40:
        x[4] = (x[4].float() / 16).round().to(BF) * 16  # a handful of distinct values: ties everywhere
    ld = (V + 8 + 7) // 8 * 8                           # a multiple of 8: with offset 0 every row is 16-byte aligned
    rows = with_sentinels(x, ld)
    check_launch(rows, launch(L, rows, V, N_CYCLE, 1), V, N_CYCLE, 1, f"V={V} aligned")
    check_launch(rows, launch(L, rows, V, N_CYCLE, 1, offset=3, raw_offset=1), V, N_CYCLE, 1, f"V={V} offset 3")
    rows = with_sentinels(x, V + 3)                     # an odd stride: the rows' alignments differ within one launch
    check_launch(rows, launch(L, rows, V, N_CYCLE, 1, raw_pad=8), V, N_CYCLE, 1, f"V={V} ld V+3")
    o = launch(L, rows, V, [5, 0, -1, 20, 1], 2, copy=False)        # rows_per_param 2, no copy
    check_launch(rows, o, V, [5, 0, -1, 20, 1], 2, f"V={V} rpp 2")


CREST = [5, 4095, 4096, 8191, 8192, 12288, 50000, 100000, 128255]


@pytest.fixture(scope="module")
def large(L):
    """The two real vocabularies: 24 rows with rows_per_param 4 (aligned) and 25 with 1 (every row offset by one entry), among them
    rows quantised to a handful of values (ties straddle the slice borders).  Launched and checked once, shared below."""
    out = {}
    for V, T, rpp, n_tops, offset in ((128256, 24, 4, [5, -1, 0, 1, 20, 20], 0),
                                      (151936, 25, 1, (N_CYCLE * 3)[:25], 1)):
        x = random_rows(T, V, V)
        for t, q in ((0, 16.0), (5, 8.0), (17, 32.0), (20, 4.0)):
            x[t] = (x[t].float() / q).round().to(BF) * q
            x[t, CREST] = 40.0                          # the row's maximum, in six slices and on both sides of two slice borders
        x[21, :] = 1.5
        rows = with_sentinels(x, V + 8)
        o = launch(L, rows, V, n_tops, rpp, offset=offset)
        out[V] = (rows, o, T, rpp, n_tops, offset)
    return out


@pytest.mark.parametrize("V", [128256, 151936])
def test_real_vocabularies(L, large, V):
    rows, o, T, rpp, n_tops, offset = large[V]
    refs = check_launch(rows, o, V, n_tops, rpp, f"V={V}")
    # the quantised rows do have ties across slice borders among their top entries: the crest in index order, then the next value's class
    t = 17 if V == 128256 else 5                        # (a quantised row with n_top = 20)
    assert refs[t].top_id[:len(CREST)] == CREST and len(set(refs[t].top_val)) == 2, refs[t].top_id
    assert o.id[t, :len(CREST)].tolist() == CREST
    print(f"V={V}: worst |lse - f64| {WORST['lse']:.3g}, worst |top logprob - f64| {WORST['top']:.3g} so far")


def test_edge_rows_of_the_header(L):
    V = 4100                                            # two slices
    x = random_rows(10, V, 7)
    nan, inf = float("nan"), float("inf")
    x[0, 5] = nan; x[0, 4097] = nan; x[0, x[0].float().nan_to_num(-99).argmax()] = nan      # NaN inside, also where the maximum was
    x[1, :] = nan                                       # nothing comparable
    x[2, 4098] = inf                                    # a +inf class of 1, in the second slice
    x[3, 7] = inf; x[3, 4000] = inf; x[3, 4099] = inf   # ... of 3, in both slices
    x[4, 100:4090] = -inf                               # -inf entries, whole 8-entry chunks of them
    x[5, :] = -inf                                      # every comparable entry -inf
    x[5, 9] = nan
    x[6, :] = -inf; x[6, 4099] = 2.0                    # one finite entry: logprob 0, then -inf entries in index order
    x[7, 0] = 0.0; x[7, 1:] = -0.0                      # +0.0 and -0.0 are one value: the top list is 0, 1, 2, ...
    x[8, :] = nan; x[8, 4097] = -1.0                    # one comparable entry: n = 1, the other slots -1 / -inf
    n_tops = [5, 3, 5, 5, 20, 4, 3, 5, 6, 0]
    rows = with_sentinels(x, V + 4)
    o = launch(L, rows, V, n_tops, 1)
    refs = check_launch(rows, o, V, n_tops, 1, "edges")
    assert np.isnan(o.lse[1]) and o.id[1, :3].tolist() == [-1, -1, -1] and np.isneginf(o.val[1, :3]).all()
    assert np.isposinf(o.lse[2]) and o.id[2, 0] == 4098 and o.val[2, 0] == 0.0 and np.isneginf(o.val[2, 1:5]).all()
    assert o.id[3, :3].tolist() == [7, 4000, 4099] and np.allclose(o.val[3, :3], -np.log(3.0), atol=1e-6) and np.isneginf(o.val[3, 3])
    assert np.isneginf(o.lse[5]) and o.id[5, :4].tolist() == [0, 1, 2, 3] and np.allclose(o.val[5, :4], -np.log(V - 1.0), atol=1e-5)
    assert o.id[6, :3].tolist() == [4099, 0, 1] and o.val[6, 0] == 0.0 and np.isneginf(o.val[6, 1:3]).all()
    assert o.id[7, :5].tolist() == [0, 1, 2, 3, 4]
    assert o.id[8, :6].tolist() == [4097, -1, -1, -1, -1, -1] and o.val[8, 0] == 0.0 and np.isneginf(o.val[8, 1:6]).all()
    assert refs[8].top_id == [4097, -1, -1, -1, -1, -1]
    # an n_top outside 0..SSD_LOGPROB_MAX_N is a skip
    o = launch(L, rows, V, [21, -5, 5, 5, 5, 5, 5, 5, 5, 5], 1)
    assert o.lse[0] == np.float32(S_LSE) and o.lse[1] == np.float32(S_LSE) and (o.id[:2] == S_ID).all() and (o.raw[:2] == S_RAW).all()


def test_pick_against_the_reference(L, large):
    V = 128256
    rows, o, T, rpp, n_tops, _ = large[V]
    x = rows[:, :V].to(torch.float64).numpy()
    g = torch.Generator().manual_seed(3)
    tokens = torch.randint(0, V, (T,), generator=g)
    tokens[1], tokens[2], tokens[3] = -1, V, V - 1
    for t in (0, 12, 16, 20):                           # (rows with n_top >= 1)
        tokens[t] = int(o.id[t, 0])
    for src, ld in ((o.d_rows, rows.shape[1]), (o.d_raw, o.raw_ld)):          # the live rows, or the copy
        out = torch.full((T,), S_OUT, dtype=torch.float32, device="cuda")
        L.logprob_pick(src, ld, T, V, tokens.cuda(), o.d_lse, o.d_ntop, rpp, out)
        torch.cuda.synchronize()
        out = out.cpu().numpy()
        for t in range(T):
            n, tok = n_tops[t // rpp], int(tokens[t])
            if n < 0:
                assert out[t] == np.float32(S_OUT), f"row {t}: a skipped row was written"
                continue
            ref = R.logprob_row(x[t], 0)
            d = close(float(out[t]), R.pick(x[t], tok, ref.lse))
            WORST["pick"] = max(WORST["pick"], d)
            assert d <= TOL, (t, out[t])
            if n >= 1 and tok == o.id[t, 0]:
                assert out[t] == o.val[t, 0], f"row {t}: the pick of the top entry is not its top value by bits"
        assert np.isnan(out[1]) and np.isnan(out[2]) and not np.isnan(out[3])
    print(f"worst |pick - f64| {WORST['pick']:.3g}; worst lse {WORST['lse']:.3g}, top {WORST['top']:.3g}")


@pytest.mark.parametrize("K1", [2, 4, 8])
def test_pick_verify_against_the_reference(L, K1):
    K, B, V = K1 - 1, 6, 4100
    T = B * K1
    x = random_rows(T, V, 50 + K1)
    rows = with_sentinels(x, V + 4)
    n_tops = [3, 0, -1, 20, 1, 0]
    o = launch(L, rows, V, n_tops, K1)
    g = torch.Generator().manual_seed(K1)
    ids = torch.randint(0, V, (B, K1), generator=g)
    accept = [0, K, K // 2, min(1, K), K, 0]            # none, all, in between; sequence 2 is skipped
    recovery = torch.randint(0, V, (B,), generator=g)
    recovery[5] = V                                     # out of range: NaN
    ids[1, 1] = -1                                      # an accepted input out of range: NaN
    out = torch.full((B, K1), S_OUT, dtype=torch.float32, device="cuda")
    L.logprob_pick_verify(o.d_rows, rows.shape[1], B, K, V, ids.cuda(), torch.tensor(accept, dtype=torch.int32, device="cuda"),
                          recovery.cuda(), o.d_lse, o.d_ntop, out)
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    x64 = x.to(torch.float64).numpy()
    for b in range(B):
        toks = R.verify_tokens(ids[b].tolist(), accept[b], int(recovery[b]))
        assert toks.count(None) == K - accept[b]
        for j in range(K1):
            t = b * K1 + j
            if n_tops[b] < 0:
                assert out[b, j] == np.float32(S_OUT)
            elif toks[j] is None:
                assert np.isnan(out[b, j]), (b, j)      # rows past the recovery row
            else:
                assert close(float(out[b, j]), R.pick(x64[t], toks[j], R.logprob_row(x64[t], 0).lse)) <= TOL, (b, j)
    assert np.isnan(out[1, 0]) and np.isnan(out[5, 0]) and not np.isnan(out[0, 0])


def test_two_runs_and_a_graph_replay_are_bit_equal(L, large):
    from ssd_amd.utils.graphs import capture
    V = 128256
    rows, a, T, rpp, n_tops, _ = large[V]
    ld = rows.shape[1]
    b = launch(L, rows, V, n_tops, rpp)
    c = launch(L, rows, V, n_tops, rpp, offset=1)       # the 2-byte path: the same bits whatever the alignment
    for o in (b, c):
        assert np.array_equal(a.lse.view(np.int32), o.lse.view(np.int32)) and np.array_equal(a.val.view(np.int32), o.val.view(np.int32))
        assert np.array_equal(a.id, o.id) and np.array_equal(a.raw, o.raw)
    o = b
    tokens = torch.zeros(T, dtype=torch.int64, device="cuda")
    out = torch.zeros(T, dtype=torch.float32, device="cuda")
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with capture(graph, stream=stream):
        L.logprob_rows(o.d_rows, ld, T, V, o.d_ntop, rpp, o.d_lse, o.d_val, o.d_id, o.d_ws, raw_copy=o.d_raw, raw_ld=o.raw_ld)
        L.logprob_pick(o.d_raw, o.raw_ld, T, V, tokens, o.d_lse, o.d_ntop, rpp, out)

    def refill():
        o.d_lse.fill_(S_LSE); o.d_val.fill_(S_VAL); o.d_id.fill_(S_ID); o.d_raw.view(torch.int16).fill_(S_RAW); out.fill_(S_OUT)

    refill()
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(o.d_lse.cpu().numpy().view(np.int32), a.lse.view(np.int32))
    assert np.array_equal(o.d_val.cpu().numpy().view(np.int32), a.val.view(np.int32)) and np.array_equal(o.d_id.cpu().numpy(), a.id)
    assert np.array_equal(bits(o.d_raw.cpu()), a.raw)
    # fresh counts on the device, no new capture: the replay follows them
    fresh = [0, 20, -1, 5, 1, -1]
    o.d_ntop.copy_(torch.tensor(fresh, dtype=torch.int32))
    refill()
    graph.replay()
    torch.cuda.synchronize()
    o.lse, o.val, o.id, o.raw = o.d_lse.cpu().numpy(), o.d_val.cpu().numpy(), o.d_id.cpu().numpy(), bits(o.d_raw.cpu())
    check_launch(rows, o, V, fresh, rpp, "replay with fresh n_top")
    got = out.cpu().numpy()
    assert all((got[t] == np.float32(S_OUT)) == (fresh[t // rpp] < 0) for t in range(T))


def test_refusals(L):
    from ssd_amd.hip.lib import SsdHipError
    z = torch.zeros(64, dtype=BF, device="cuda").view(2, 32)
    f = torch.zeros(64, dtype=torch.float32, device="cuda")
    i = torch.zeros(64, dtype=torch.int32, device="cuda")
    n0 = L.LAUNCHES
    for kw in (dict(T=0), dict(V=0), dict(rpp=0), dict(ld=16), dict(raw_ld=16)):
        a = dict(dict(ld=32, T=2, V=32, rpp=1, raw_ld=32), **kw)
        with pytest.raises(SsdHipError):
            L.logprob_rows(z, a["ld"], a["T"], a["V"], i, a["rpp"], f, f, i, f, raw_copy=z, raw_ld=a["raw_ld"])
    with pytest.raises(SsdHipError):
        L.logprob_rows(z, 32, 2, 32, i, 1, f, None, i, f)
    with pytest.raises(SsdHipError):
        L.logprob_rows_ws_bytes(1, L.MAX_V + 8)
    assert L.LAUNCHES == n0 + 6                         # the counter counts calls; none of these reached a launch

"""The mixture-of-experts kernels on the MI355X through the C ABI (csrc/moe.hip, include/ssd_hip_moe.h): ssd_moe_route, ssd_moe_gemm
and ssd_moe_combine against the float64 reference of tests/moe_ref.py.

Every output is filled with a sentinel before a launch and has a sentinel tail; everything that must not be read is bf16 NaN: the
logit columns past E, the x / act rows past the ones an entry names, and the tables of the experts no row chose.  Bars: route ids,
offs and perm bit-equal, weights within 1 bf16 ulp on at most 2 % of the entries; the GEMM outputs at the bar of test_hip_lora.py
(1 bf16 ulp of float64, differences below 2^-20 * sum|x w| exempt; moe_ref.assert_act_within_bar carries it through SiLU * mul), the
down GEMM from the kernel's OWN act; the combine bit-equal from the kernel's own d."""
import pytest
import torch

from tests import moe_ref as R
from tests.util import assert_close_bf16

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
SENT = 0x7fc1           # a bf16 NaN pattern no kernel produces (f2bf quiets to ...40)
ISENT = -77
NAN = float("nan")
_TABLES = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda")


def _route(logits, E, k, norm, pad=5):
    """ssd_moe_route on bf16 rows [T][ld] -> (ids [T, k], w fp32 [T, k], offs, perm), each launched into a sentinel-filled buffer with
    a sentinel tail that must survive."""
    from ssd_amd.hip import moe_ops as M
    T, ld = logits.shape
    dev = logits.device
    ids = torch.full((T * k + pad,), ISENT, dtype=torch.int32, device=dev)
    w = torch.full((T * k + pad,), NAN, dtype=torch.float32, device=dev)
    offs = torch.full((E + 1 + pad,), ISENT, dtype=torch.int32, device=dev)
    perm = torch.full((T * k + pad,), ISENT, dtype=torch.int32, device=dev)
    M.moe_route(logits, ld, T, E, k, norm, ids, w, offs, perm)
    torch.cuda.synchronize()
    assert bool((ids[T * k:] == ISENT).all() and (offs[E + 1:] == ISENT).all() and (perm[T * k:] == ISENT).all()), "route wrote past its outputs"
    assert bool(torch.isnan(w[T * k:]).all()), "route wrote past topk_w"
    return ids[:T * k].view(T, k), w[:T * k].view(T, k), offs[:E + 1], perm[:T * k]


def _logits(T, E, ld, seed, dev):
    """bf16 rows on a grid of quarters (exact ties everywhere, also at the k-th boundary), one all-equal row, NaN past E."""
    g = torch.Generator(device=dev).manual_seed(seed)
    l = torch.randint(-12, 13, (T, ld), generator=g, device=dev).float() / 4
    fine = torch.randn(T, ld, generator=g, device=dev)
    l = torch.where(torch.arange(T, device=dev)[:, None] % 3 == 2, fine * 2, l)      # every third row: distinct values
    l[T // 2] = 1.25
    l = l.to(BF)
    l[:, E:] = NAN
    return l


ROUTE_CASES = [(8, 1, 1), (8, 2, 7), (8, 8, 16), (128, 1, 17), (128, 2, 33), (128, 8, 130), (256, 1, 2049), (256, 2, 16), (256, 8, 2049),
               (8, 8, 2049), (128, 8, 1), (256, 8, 7), (128, 2, 2049), (8, 2, 130), (256, 2, 33), (128, 1, 16), (8, 1, 17)]


@pytest.mark.parametrize("E,k,T", ROUTE_CASES)
def test_route(dev, E, k, T):
    for ld, norm in ((E + 8, True), (E, False), (E + 8, False)):
        l = _logits(T, E, ld, seed=E * 31 + k * 7 + T + ld, dev=dev)
        ids, w, offs, perm = _route(l, E, k, norm)
        want_ids, want_w, want_offs, want_perm = R.route_ref(l[:, :E], k, norm)
        what = f"E={E} k={k} T={T} ld={ld} norm={norm}"
        assert torch.equal(ids, want_ids), f"{what}: topk_ids"
        assert torch.equal(offs, want_offs) and int(offs[E]) == T * k, f"{what}: offs"
        assert torch.equal(perm, want_perm), f"{what}: perm"
        assert torch.equal(w, w.to(BF).float()), f"{what}: a weight is not a bf16 value"
        assert_close_bf16(w.to(BF), want_w, max_ulp=1, max_frac=0.02, what=what)
        if k < E:       # the logits do hold exact ties at the boundary
            top = torch.sort(l[:, :E].float(), dim=-1, descending=True).values
            assert bool((top[:, k - 1] == top[:, k]).any()), f"{what}: input problem, no tie at the k-th boundary"


def _frag_tables(W, mode):
    from ssd_amd.hip import ops as H
    E, N, K = W.shape
    out = torch.empty(E * N * K, dtype=BF, device=W.device)
    for e in range(E):
        H.rows_to_frag(W[e].contiguous(), out[e * N * K:(e + 1) * N * K], N, K, mode)
    return out


def _tables(E, K, I, Hd, dev):
    """Expert weights and their fragment-major tables, generated once per geometry and never modified."""
    key = (E, K, I, Hd)
    if key not in _TABLES:
        g = torch.Generator(device=dev).manual_seed(E + K + I + Hd)
        Wgu = (torch.randn(E, 2 * I, K, generator=g, device=dev) / K ** 0.5).to(BF)
        Wd = (torch.randn(E, Hd, I, generator=g, device=dev) / I ** 0.5).to(BF)
        _TABLES.clear()         # one geometry at a time: the largest is 2.4 GB with its tables
        _TABLES[key] = (Wgu, Wd, _frag_tables(Wgu, 1), _frag_tables(Wd, 0))
        torch.cuda.synchronize()
    return _TABLES[key]


def _routing(kind, T, k, E, dev):
    """Hand-made topk ids [T, k] (distinct within a row)."""
    ar = torch.arange(T, device=dev)
    if kind == "one":           # every row on the same k experts: T rows per expert, several row tiles and a ragged last one
        return (torch.arange(k, device=dev) * (E // k) + E // k - 1).repeat(T, 1)
    if kind == "16_17":         # exactly 16 rows on one expert, exactly 17 on another (k == 1, T == 33)
        assert k == 1 and T == 33
        return torch.where(ar < 16, 1, E - 2).view(T, 1)
    if kind == "distinct":      # one row on each of T * k distinct experts
        assert T * k <= E
        g = torch.Generator(device=dev).manual_seed(T + k)
        return torch.randperm(E, generator=g, device=dev)[:T * k].view(T, k)
    if kind == "few":           # most experts empty: the rows share k + 1 experts
        pool = torch.arange(k + 1, device=dev) * (E // (k + 1))
        return torch.stack([pool[(torch.arange(k, device=dev) + t) % (k + 1)] for t in range(T)])
    assert kind == "random"
    g = torch.Generator(device=dev).manual_seed(T * k + E)
    return torch.rand(T, E, generator=g, device=dev).topk(k, dim=-1).indices


def _nan_unchosen(tab, ids, E):
    """A copy of the tables with every expert no row chose turned into bf16 NaN."""
    out = tab.clone().view(E, -1)
    chosen = torch.zeros(E, dtype=torch.bool, device=tab.device)
    chosen[ids.reshape(-1).long()] = True
    out[~chosen] = NAN
    return out.view(-1)


def _run_block(dev, K, I, Hd, E, k, T, kind, what):
    from ssd_amd.hip import moe_ops as M
    Wgu, Wd, gu_tab, d_tab = _tables(E, K, I, Hd, dev)
    ids = _routing(kind, T, k, E, dev).int()
    assert all(len(set(r)) == k for r in ids.tolist()), "input problem: a row names an expert twice"
    offs, perm = R.group_tables(ids, E)
    g = torch.Generator(device=dev).manual_seed(T + K + k)
    n = T * k
    x = torch.full((T + 3, K), NAN, dtype=BF, device=dev)         # the rows past T: nobody names them
    x[:T] = torch.randn(T, K, generator=g, device=dev).to(BF)
    act = torch.full((n + 3, I), SENT, dtype=torch.int16, device=dev)
    d = torch.full((n + 3, Hd), SENT, dtype=torch.int16, device=dev)
    gu_nan, d_nan = _nan_unchosen(gu_tab, ids, E), _nan_unchosen(d_tab, ids, E)
    M.moe_gemm(x, gu_nan, offs, perm, act, T, k, E, 2 * I, K, M.EPI_UP)
    M.moe_gemm(act, d_nan, offs, perm, d, T, k, E, Hd, I, M.EPI_DOWN)
    torch.cuda.synchronize()
    assert bool((act[n:] == SENT).all() and (d[n:] == SENT).all()), f"{what}: a write past the T * k entries"
    act_b, d_b = act[:n].view(BF), d[:n].view(BF)
    assert bool(torch.isfinite(act_b.float()).all() and torch.isfinite(d_b.float()).all()), f"{what}: an entry was not written, or NaN leaked in"
    gu64, gumag = R.grouped_exact(x[:T], Wgu, ids, gather_tokens=True)
    R.assert_act_within_bar(act_b, gu64[:, :I], gumag[:, :I], gu64[:, I:], gumag[:, I:], f"{what} act")
    d64, dmag = R.grouped_exact(act_b, Wd, ids, gather_tokens=False)
    R.assert_within_bar(d_b, d64, dmag, f"{what} d")
    # combine, from the kernel's own d
    w = torch.rand(T, k, generator=g, device=dev).to(BF).float()
    h = torch.full((T + 3, Hd), SENT, dtype=torch.int16, device=dev)
    M.moe_combine(d, w, h, T, k, Hd)
    torch.cuda.synchronize()
    assert bool((h[T:] == SENT).all()), f"{what}: combine wrote past T rows"
    assert torch.equal(h[:T].view(BF).view(torch.int16), R.combine_ref(d_b, w).view(torch.int16)), f"{what}: combine"
    return act, d, h


SMALL, BIG, ODD = (64, 32, 64), (2048, 768, 2048), (2080, 96, 2064)
GEMM_CASES = [
    (SMALL, 8, 1, 33, "one"), (SMALL, 8, 2, 130, "one"), (SMALL, 8, 1, 33, "16_17"), (SMALL, 8, 2, 4, "distinct"), (SMALL, 8, 8, 17, "one"),
    (SMALL, 8, 8, 1, "distinct"), (SMALL, 8, 2, 7, "few"), (SMALL, 128, 8, 16, "distinct"), (SMALL, 128, 2, 130, "random"),
    (ODD, 8, 2, 33, "one"), (ODD, 8, 1, 33, "16_17"), (ODD, 8, 8, 130, "one"), (ODD, 128, 8, 17, "random"), (ODD, 128, 1, 130, "one"),
    (ODD, 128, 2, 7, "few"), (ODD, 128, 8, 8, "distinct"),
    (BIG, 8, 2, 33, "one"), (BIG, 8, 1, 33, "16_17"), (BIG, 8, 8, 1, "distinct"),
    (BIG, 128, 8, 8, "distinct"), (BIG, 128, 8, 130, "random"), (BIG, 128, 1, 130, "one"), (BIG, 128, 2, 7, "few"), (BIG, 128, 1, 33, "16_17"),
]


@pytest.mark.parametrize("shape,E,k,T,kind", GEMM_CASES)
def test_gemm_and_combine(dev, shape, E, k, T, kind):
    K, I, Hd = shape
    _run_block(dev, K, I, Hd, E, k, T, kind, f"K={K} I={I} H={Hd} E={E} k={k} T={T} {kind}")


def test_two_runs_give_equal_bits(dev):
    K, I, Hd = ODD
    a = _run_block(dev, K, I, Hd, 128, 8, 130, "random", "run a")
    b = _run_block(dev, K, I, Hd, 128, 8, 130, "random", "run b")
    assert all(torch.equal(p, q) for p, q in zip(a, b))


def test_graph_capture_replays_other_routes(dev):
    """route + up + down + combine captured once; the replay with other logits -- other routes -- in the same buffers equals the
    eager launches by bits."""
    from ssd_amd.hip import moe_ops as M
    K, I, Hd = SMALL
    E, k, T = 128, 8, 24
    Wgu, Wd, gu_tab, d_tab = _tables(E, K, I, Hd, dev)
    g = torch.Generator(device=dev).manual_seed(5)
    x = torch.randn(T, K, generator=g, device=dev).to(BF)
    logits = torch.zeros(T, E, dtype=BF, device=dev)
    ids = torch.zeros(T * k, dtype=torch.int32, device=dev)
    w = torch.zeros(T * k, dtype=torch.float32, device=dev)
    offs = torch.zeros(E + 1, dtype=torch.int32, device=dev)
    perm = torch.zeros(T * k, dtype=torch.int32, device=dev)
    act = torch.zeros(T * k, I, dtype=BF, device=dev)
    d = torch.zeros(T * k, Hd, dtype=BF, device=dev)
    h = torch.zeros(T, Hd, dtype=BF, device=dev)

    def block():
        M.moe_route(logits, E, T, E, k, True, ids, w, offs, perm)
        M.moe_gemm(x, gu_tab, offs, perm, act, T, k, E, 2 * I, K, M.EPI_UP)
        M.moe_gemm(act, d_tab, offs, perm, d, T, k, E, Hd, I, M.EPI_DOWN)
        M.moe_combine(d, w, h, T, k, Hd)

    la = torch.randn(T, E, generator=g, device=dev).to(BF)
    lb = torch.randn(T, E, generator=g, device=dev).to(BF)
    eager = {}
    for name, l in (("a", la), ("b", lb)):
        logits.copy_(l)
        block()
        torch.cuda.synchronize()
        eager[name] = [t.clone() for t in (ids, w, offs, perm, act, d, h)]
    assert not torch.equal(eager["a"][0], eager["b"][0]), "input problem: the two logit sets route alike"
    logits.copy_(la)
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        block()                                                 # warm-up on the capture stream
        with torch.cuda.graph(graph, stream=s):
            block()
    torch.cuda.current_stream().wait_stream(s)
    for name, l in (("b", lb), ("a", la), ("b", lb)):
        for t in (ids, perm, offs):
            t.fill_(ISENT)
        for t in (act, d, h):
            t.fill_(NAN)
        logits.copy_(l)
        graph.replay()
        torch.cuda.synchronize()
        for got, want, what in zip((ids, w, offs, perm, act, d, h), eager[name], ("ids", "w", "offs", "perm", "act", "d", "h")):
            assert torch.equal(got.view(torch.int16) if got.dtype == BF else got, want.view(torch.int16) if want.dtype == BF else want), \
                f"replay with logits {name}: {what} differs from the eager launch"


def test_refusals(dev):
    """Every SSD_ERR_* the header promises, before any launch (the outputs keep their bits)."""
    from ssd_amd.hip import moe_ops as M
    from ssd_amd.hip.ops import _p, _stream
    lib = M.load_moe_library()
    OK, SHAPE, ARG = 0, -1, -3
    E, k, T, K, I, Hd = 8, 2, 4, 64, 32, 64
    l = torch.randn(T, E, device=dev).to(BF)
    ids = torch.full((T * k,), ISENT, dtype=torch.int32, device=dev)
    w = torch.zeros(T * k, dtype=torch.float32, device=dev)
    offs = torch.full((E + 1,), ISENT, dtype=torch.int32, device=dev)
    perm = torch.full((T * k,), ISENT, dtype=torch.int32, device=dev)

    def route(**kw):
        a = dict(logits=_p(l), ld=E, T=T, E=E, k=k, norm=1, ids=_p(ids), w=_p(w), offs=_p(offs), perm=_p(perm))
        a.update(kw)
        return lib.ssd_moe_route(a["logits"], a["ld"], a["T"], a["E"], a["k"], a["norm"], a["ids"], a["w"], a["offs"], a["perm"], _stream())

    for kw, rc in ((dict(logits=0), ARG), (dict(ids=0), ARG), (dict(w=0), ARG), (dict(offs=0), ARG), (dict(perm=0), ARG),
                   (dict(T=0), SHAPE), (dict(k=0), SHAPE), (dict(k=9), SHAPE), (dict(E=4, k=2), SHAPE), (dict(E=12), SHAPE),
                   (dict(E=264, ld=264), SHAPE), (dict(ld=E - 1), SHAPE), (dict(T=(1 << 24) // k + 1), SHAPE)):
        assert route(**kw) == rc, kw
    torch.cuda.synchronize()
    assert bool((ids == ISENT).all() and (offs == ISENT).all() and (perm == ISENT).all()), "a refused call launched"
    assert route() == OK
    x = torch.randn(T, K, device=dev).to(BF)
    gu = torch.zeros(E * 2 * I * K, dtype=BF, device=dev)
    dn = torch.zeros(E * Hd * I, dtype=BF, device=dev)
    act = torch.full((T * k, I), SENT, dtype=torch.int16, device=dev)
    d = torch.full((T * k, Hd), SENT, dtype=torch.int16, device=dev)

    def gemm(**kw):
        a = dict(rows=_p(x), tab=_p(gu), offs=_p(offs), perm=_p(perm), out=_p(act), T=T, k=k, E=E, N=2 * I, K=K, epi=M.EPI_UP)
        a.update(kw)
        return lib.ssd_moe_gemm(a["rows"], a["tab"], a["offs"], a["perm"], a["out"], a["T"], a["k"], a["E"], a["N"], a["K"], a["epi"], _stream())

    for kw, rc in ((dict(rows=0), ARG), (dict(tab=0), ARG), (dict(offs=0), ARG), (dict(perm=0), ARG), (dict(out=0), ARG), (dict(epi=2), ARG),
                   (dict(epi=-1), ARG), (dict(T=0), SHAPE), (dict(k=0), SHAPE), (dict(k=9), SHAPE), (dict(E=4), SHAPE), (dict(E=20), SHAPE),
                   (dict(E=512), SHAPE), (dict(K=48), SHAPE), (dict(K=0), SHAPE), (dict(N=32), SHAPE), (dict(N=96), SHAPE), (dict(N=0), SHAPE),
                   (dict(epi=M.EPI_DOWN, N=24), SHAPE), (dict(epi=M.EPI_DOWN, N=Hd, K=I + 8), SHAPE)):
        assert gemm(**kw) == rc, kw
    torch.cuda.synchronize()
    assert bool((act == SENT).all()), "a refused call launched"
    assert gemm() == OK
    assert gemm(epi=M.EPI_DOWN, rows=_p(act), tab=_p(dn), out=_p(d), N=Hd, K=I) == OK
    h = torch.full((T, Hd), SENT, dtype=torch.int16, device=dev)

    def combine(**kw):
        a = dict(d=_p(d), w=_p(w), h=_p(h), T=T, k=k, H=Hd)
        a.update(kw)
        return lib.ssd_moe_combine(a["d"], a["w"], a["h"], a["T"], a["k"], a["H"], _stream())

    for kw, rc in ((dict(d=0), ARG), (dict(w=0), ARG), (dict(h=0), ARG), (dict(T=0), SHAPE), (dict(k=0), SHAPE), (dict(k=9), SHAPE),
                   (dict(H=24), SHAPE), (dict(H=0), SHAPE)):
        assert combine(**kw) == rc, kw
    torch.cuda.synchronize()
    assert bool((h == SENT).all()), "a refused call launched"
    assert combine() == OK
    torch.cuda.synchronize()

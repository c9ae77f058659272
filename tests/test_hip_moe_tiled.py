"""ssd_moe_gemm_tiled (csrc/moe_tiled.hip, include/ssd_hip_moe_tiled.h) on the MI355X against the float64 reference of
tests/moe_ref.py, at the bars of tests/test_hip_moe.py (whose tables, routings and sentinels these tests share): up and down within
1 bf16 ulp of float64 (differences below 2^-20 * sum|x w| exempt), the down GEMM from the kernel's own act.  Everything that must not
be read is bf16 NaN (the tables of unchosen experts, the x rows past T), the outputs have sentinel tails.  BM is 128: the routings
put BM + 1 and exactly BM rows on an expert."""
import pytest
import torch

from tests import moe_ref as R
from tests.test_hip_moe import BF, BIG, NAN, ODD, SENT, SMALL, _nan_unchosen, _routing, _tables, dev  # noqa: F401

pytestmark = pytest.mark.gpu


def _run(dev, shape, E, ids, x):
    """up then down on the tiled kernel for the routes ids [T, k] and rows x [T + pad, K] -> (act, d) with their sentinel tails."""
    from ssd_amd.hip import moe_ops as M
    K, I, Hd = shape
    T, k = ids.shape
    n = T * k
    _, _, gu_tab, d_tab = _tables(E, K, I, Hd, dev)
    offs, perm = R.group_tables(ids, E)
    act = torch.full((n + 3, I), SENT, dtype=torch.int16, device=dev)
    d = torch.full((n + 3, Hd), SENT, dtype=torch.int16, device=dev)
    M.moe_gemm_tiled(x, _nan_unchosen(gu_tab, ids, E), offs, perm, act, T, k, E, 2 * I, K, M.EPI_UP)
    M.moe_gemm_tiled(act, _nan_unchosen(d_tab, ids, E), offs, perm, d, T, k, E, Hd, I, M.EPI_DOWN)
    torch.cuda.synchronize()
    return act, d


def _rows(T, K, seed, dev):
    x = torch.full((T + 3, K), NAN, dtype=BF, device=dev)         # the rows past T: nobody names them
    x[:T] = torch.randn(T, K, generator=torch.Generator(device=dev).manual_seed(seed), device=dev).to(BF)
    return x


CASES = [
    (SMALL, 8, 2, 129, "one"), (SMALL, 8, 2, 128, "one"), (SMALL, 8, 1, 33, "16_17"), (SMALL, 8, 2, 7, "few"), (SMALL, 8, 8, 1, "distinct"),
    (SMALL, 128, 8, 130, "random"),
    (ODD, 8, 2, 129, "one"), (ODD, 8, 2, 128, "one"), (ODD, 8, 1, 33, "16_17"), (ODD, 128, 2, 7, "few"), (ODD, 8, 8, 1, "distinct"),
    (BIG, 128, 8, 130, "random"),
]


@pytest.mark.parametrize("shape,E,k,T,kind", CASES)
def test_up_and_down(dev, shape, E, k, T, kind):
    K, I, Hd = shape
    what = f"K={K} I={I} H={Hd} E={E} k={k} T={T} {kind}"
    Wgu, Wd, _, _ = _tables(E, K, I, Hd, dev)
    ids = _routing(kind, T, k, E, dev).int()
    x = _rows(T, K, T + K + k, dev)
    n = T * k
    act, d = _run(dev, shape, E, ids, x)
    assert bool((act[n:] == SENT).all() and (d[n:] == SENT).all()), f"{what}: a write past the T * k entries"
    act_b, d_b = act[:n].view(BF), d[:n].view(BF)
    assert bool(torch.isfinite(act_b.float()).all() and torch.isfinite(d_b.float()).all()), f"{what}: an entry was not written, or NaN leaked in"
    gu64, gumag = R.grouped_exact(x[:T], Wgu, ids, gather_tokens=True)
    R.assert_act_within_bar(act_b, gu64[:, :I], gumag[:, :I], gu64[:, I:], gumag[:, I:], f"{what} act")
    d64, dmag = R.grouped_exact(act_b, Wd, ids, gather_tokens=False)
    R.assert_within_bar(d_b, d64, dmag, f"{what} d")
    again = _run(dev, shape, E, ids, x)
    assert torch.equal(act, again[0]) and torch.equal(d, again[1]), f"{what}: two runs differ by bits"


def test_a_row_alone_gives_the_same_bits(dev):
    """The normative order: an entry's result depends on its own row and its expert only -- not on T, its place in a block or the
    other rows' routes.  One row of the T = 130 random case, run alone at T = 1 with its expert ids."""
    E, k, T, t = 128, 8, 130, 77
    ids = _routing("random", T, k, E, dev).int()
    x = _rows(T, BIG[0], 5, dev)
    act, d = _run(dev, BIG, E, ids, x)
    x1 = _rows(1, BIG[0], 6, dev)
    x1[0] = x[t]
    act1, d1 = _run(dev, BIG, E, ids[t:t + 1].contiguous(), x1)
    assert torch.equal(act1[:k], act[t * k:(t + 1) * k]) and torch.equal(d1[:k], d[t * k:(t + 1) * k])


def test_graph_capture_replays_other_routes(dev):
    """up + down captured once; replays after offs / perm / x were rewritten in place with other routes equal the eager launches."""
    from ssd_amd.hip import moe_ops as M
    K, I, Hd = SMALL
    E, k, T = 128, 8, 40
    _, _, gu_tab, d_tab = _tables(E, K, I, Hd, dev)
    x, offs, perm = _rows(T, K, 1, dev), torch.zeros(E + 1, dtype=torch.int32, device=dev), torch.zeros(T * k, dtype=torch.int32, device=dev)
    act = torch.zeros(T * k, I, dtype=BF, device=dev)
    d = torch.zeros(T * k, Hd, dtype=BF, device=dev)

    def block():
        M.moe_gemm_tiled(x, gu_tab, offs, perm, act, T, k, E, 2 * I, K, M.EPI_UP)
        M.moe_gemm_tiled(act, d_tab, offs, perm, d, T, k, E, Hd, I, M.EPI_DOWN)

    def put(name):
        kind, seed = ("random", 2) if name == "a" else ("few", 3)
        o, p = R.group_tables(_routing(kind, T, k, E, dev).int(), E)
        offs.copy_(o), perm.copy_(p), x.copy_(_rows(T, K, seed, dev))

    eager = {}
    for name in "ab":
        put(name)
        block()
        torch.cuda.synchronize()
        eager[name] = (act.clone(), d.clone())
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        block()                                                 # warm-up on the capture stream
        with torch.cuda.graph(graph, stream=s):
            block()
    torch.cuda.current_stream().wait_stream(s)
    for name in "bab":
        put(name)
        act.fill_(NAN), d.fill_(NAN)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(act.view(torch.int16), eager[name][0].view(torch.int16)), f"replay {name}: act differs from the eager launch"
        assert torch.equal(d.view(torch.int16), eager[name][1].view(torch.int16)), f"replay {name}: d differs from the eager launch"


OK, SHAPE, ARG = 0, -1, -3
REFUSALS = [(dict(rows=0), ARG), (dict(tab=0), ARG), (dict(offs=0), ARG), (dict(perm=0), ARG), (dict(out=0), ARG), (dict(epi=2), ARG),
            (dict(epi=-1), ARG), (dict(T=0), SHAPE), (dict(k=0), SHAPE), (dict(k=9), SHAPE),
            (dict(E=4), SHAPE), (dict(E=20), SHAPE), (dict(E=512), SHAPE), (dict(K=48), SHAPE), (dict(K=0), SHAPE), (dict(N=32), SHAPE),
            (dict(N=96), SHAPE), (dict(N=0), SHAPE), (dict(T=(1 << 24) // 2 + 1), SHAPE), (dict(epi=1, N=24), SHAPE),
            (dict(epi=1, N=64, K=40), SHAPE), (dict(), OK)]


@pytest.mark.parametrize("kw,rc", REFUSALS)
def test_refusals(dev, kw, rc):
    """Every SSD_ERR_* the header promises, before any launch (the output keeps its bits)."""
    from ssd_amd.hip import moe_ops as M
    from ssd_amd.hip.ops import _p, _stream
    E, k, T, K, I = 8, 2, 4, 64, 32
    x = torch.randn(T, K, device=dev).to(BF)
    gu = torch.zeros(E * 2 * I * K, dtype=BF, device=dev)
    offs, perm = R.group_tables(_routing("one", T, k, E, dev).int(), E)
    act = torch.full((T * k, I), SENT, dtype=torch.int16, device=dev)
    a = dict(rows=_p(x), tab=_p(gu), offs=_p(offs), perm=_p(perm), out=_p(act), T=T, k=k, E=E, N=2 * I, K=K, epi=M.EPI_UP)
    a.update(kw)
    got = M.load_moe_tiled_library().ssd_moe_gemm_tiled(a["rows"], a["tab"], a["offs"], a["perm"], a["out"], a["T"], a["k"], a["E"], a["N"],
                                                        a["K"], a["epi"], _stream())
    torch.cuda.synchronize()
    assert got == rc, kw
    assert bool((act == SENT).all()) == (rc != OK), "a refused call launched"

"""ssd_moe_gemm_tiled_fp8b (csrc/moe_tiled.hip, include/ssd_hip_moe_tiled_fp8b.h) on the MI355X against moe_ref.grouped_exact over
W = s * e4m3(q) (exact in float64), at the bars, tables and poisoning of tests/test_hip_moe_fp8b.py: down from the kernel's own act; x
rows past T NaN, sentinel tails, unchosen experts' codes 0x7F and scales NaN, distinct full-mantissa scales per (group, block).  BM is 128."""
import pytest
import torch

from tests import moe_ref as R
from tests.test_hip_moe import BF, NAN, SENT, _routing
from tests.test_hip_moe_fp8b import _poison_unchosen, _tables, dev  # noqa: F401
from tests.test_hip_moe_mxfp4 import BIG, ONE, RAGGED, _x
from tests.test_hip_moe_tiled_mxfp4 import ROUTES

pytestmark = pytest.mark.gpu


def _run(dev, shape, E, ids, x):
    """up then down -> (act, d) int16 with sentinel tails."""
    from ssd_amd.hip import moe_ops as M
    K, I, Hd = shape
    _, gq, gs, _, dq, ds = _tables(E, K, I, Hd, dev)
    (T, k), n = ids.shape, ids.numel()
    offs, perm = R.group_tables(ids, E)
    xp = torch.full((T + 3, K), NAN, dtype=BF, device=dev)        # the rows past T: nobody names them
    xp[:T] = x
    act, d = (torch.full((n + 3, w), SENT, dtype=torch.int16, device=dev) for w in (I, Hd))
    for q, s, rows, out, N, Kc, epi in ((gq, gs, xp, act, 2 * I, K, M.EPI_UP), (dq, ds, act, d, Hd, I, M.EPI_DOWN)):
        M.moe_gemm_tiled_fp8b(rows, _poison_unchosen(q, ids, E, 0x7F), _poison_unchosen(s, ids, E, NAN), offs, perm, out, T, k, E, N, Kc, epi)
    torch.cuda.synchronize()
    return act, d


@pytest.mark.parametrize("shape,E,k,T,kind", [(s, *r) for s in (ONE, RAGGED) for r in ROUTES] + [(BIG, 128, 8, 130, "random")])
def test_up_and_down(dev, shape, E, k, T, kind):
    (K, I, Hd), what = shape, f"{shape} E={E} k={k} T={T} {kind}"
    Wgu, _, _, Wd, _, _ = _tables(E, K, I, Hd, dev)
    ids, x, n = _routing(kind, T, k, E, dev).int(), _x(T, K, T + K + k, dev), T * k
    act, d = _run(dev, shape, E, ids, x)
    assert bool((act[n:] == SENT).all() and (d[n:] == SENT).all()), f"{what}: a write past the T * k entries"
    act_b, d_b = act[:n].view(BF), d[:n].view(BF)
    assert bool(torch.isfinite(act_b.float()).all() and torch.isfinite(d_b.float()).all()), f"{what}: an entry was not written, or poison leaked in"
    gu64, gumag = R.grouped_exact(x, Wgu, ids, gather_tokens=True)
    R.assert_act_within_bar(act_b, gu64[:, :I], gumag[:, :I], gu64[:, I:], gumag[:, I:], f"{what} act")
    d64, dmag = R.grouped_exact(act_b, Wd, ids, gather_tokens=False)
    R.assert_within_bar(d_b, d64, dmag, f"{what} d")


def test_a_row_alone_gives_the_same_bits(dev):
    """An entry's result depends on its own row and its expert only: row 77 of the T = 130 random case, alone at T = 1."""
    E, k, T, t = 128, 8, 130, 77
    ids, x = _routing("random", T, k, E, dev).int(), _x(T, BIG[0], 5, dev)
    act, d = _run(dev, BIG, E, ids, x)
    act1, d1 = _run(dev, BIG, E, ids[t:t + 1].contiguous(), x[t:t + 1])
    assert torch.equal(act1[:k], act[t * k:(t + 1) * k]) and torch.equal(d1[:k], d[t * k:(t + 1) * k])


def test_two_runs_give_the_same_bits(dev):
    ids, x = _routing("random", 130, 8, 128, dev).int(), _x(130, RAGGED[0], 7, dev)
    (act, d), again = _run(dev, RAGGED, 128, ids, x), _run(dev, RAGGED, 128, ids, x)
    assert torch.equal(act, again[0]) and torch.equal(d, again[1])


def test_graph_capture_replays_other_routes(dev):
    """up + down captured once; replays after offs / perm / x were rewritten in place with other routes equal the eager launches."""
    from ssd_amd.hip import moe_ops as M
    (K, I, Hd), E, k, T = RAGGED, 128, 8, 40
    _, gq, gs, _, dq, ds = _tables(E, K, I, Hd, dev)
    x, offs, perm = _x(T, K, 1, dev), torch.zeros(E + 1, dtype=torch.int32, device=dev), torch.zeros(T * k, dtype=torch.int32, device=dev)
    act, d = torch.zeros(T * k, I, dtype=BF, device=dev), torch.zeros(T * k, Hd, dtype=BF, device=dev)

    def block():
        M.moe_gemm_tiled_fp8b(x, gq, gs, offs, perm, act, T, k, E, 2 * I, K, M.EPI_UP)
        M.moe_gemm_tiled_fp8b(act, dq, ds, offs, perm, d, T, k, E, Hd, I, M.EPI_DOWN)

    def run(name, launch):
        kind, seed = ("random", 2) if name == "a" else ("few", 3)
        o, p = R.group_tables(_routing(kind, T, k, E, dev).int(), E)
        offs.copy_(o), perm.copy_(p), x.copy_(_x(T, K, seed, dev)), act.fill_(NAN), d.fill_(NAN)
        launch()
        torch.cuda.synchronize()
        return torch.cat((act, d), dim=1).view(torch.int16).clone()

    eager = {name: run(name, block) for name in "ab"}
    graph, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        block()                                                 # warm-up on the capture stream
        with torch.cuda.graph(graph, stream=s):
            block()
    torch.cuda.current_stream().wait_stream(s)
    for name in "bab":
        assert torch.equal(run(name, graph.replay), eager[name]), f"replay {name} differs from the eager launch"


OK, SHAPE, ARG = 0, -1, -3
REFUSALS = [(dict([(n, 0)]), ARG) for n in ("rows", "q", "s", "offs", "perm", "out")] + [(dict(epi=2), ARG), (dict(epi=-1), ARG)]
REFUSALS += [(kw, SHAPE) for kw in (dict(T=0), dict(k=0), dict(k=9), dict(E=4), dict(E=20), dict(E=512), dict(K=64), dict(K=160),
                                    dict(N=32), dict(N=96), dict(epi=1, N=24))] + [(dict(), OK)]


@pytest.mark.parametrize("kw,rc", REFUSALS)
def test_refusals(dev, kw, rc):
    """Every SSD_ERR_* the header promises, before any launch (the output keeps its sentinel exactly when the call was refused)."""
    from ssd_amd.hip import moe_ops as M
    from ssd_amd.hip.ops import _p, _stream
    E, k, T, K, I = 8, 2, 4, 128, 128
    offs, perm = R.group_tables(_routing("few", T, k, E, dev), E)
    x, q = torch.zeros(T, K, dtype=BF, device=dev), torch.zeros(E * 2 * I * K, dtype=torch.uint8, device=dev)
    s = torch.ones(E * (2 * I // 16) * (K // 128), dtype=torch.float32, device=dev)
    act = torch.full((T * k, I), SENT, dtype=torch.int16, device=dev)
    a = dict(dict(rows=_p(x), q=_p(q), s=_p(s), offs=_p(offs), perm=_p(perm), out=_p(act), T=T, k=k, E=E, N=2 * I, K=K, epi=M.EPI_UP), **kw)
    assert M.load_moe_tiled_fp8b_library().ssd_moe_gemm_tiled_fp8b(*a.values(), _stream()) == rc, kw
    torch.cuda.synchronize()
    assert bool((act == SENT).all()) == (rc != OK), "a refused call launched (or the accepted one did not)"

"""The grouped block-scaled FP8 expert GEMM on the MI355X through the C ABI (csrc/moe_fp8b.hip, include/ssd_hip_moe_fp8b.h) against
moe_ref.grouped_exact over the float64 image s * e4m3(q) (exact in float64), both epilogues chained (act into down).

Poisoning in every case: x rows past T are NaN, outputs are sentinel-filled with a sentinel tail, the codes of every expert no row
chose are 0x7F bytes (e4m3fn NaN) and its scales NaN; the scales are 2^U(-9,-5) * U(1,2), distinct per (16-row group, block) with
full mantissas, so a wrong index or a scale applied per row or per 64 columns shows; the random codes avoid 0x7F / 0xFF.  Bars: those
of tests/test_hip_moe.py (1 bf16 ulp of the float64 value, differences below 2^-20 * sum|x w| exempt; the down GEMM from the kernel's
OWN act)."""
import pytest
import torch

from tests import moe_ref as R
from tests.test_hip_moe import _routing, SENT, NAN, BF
# the shapes (one block: a wave without work | 5 and 3 blocks, 13 down row groups | the 30B shape), T / k / E / route table and rows of the mxfp4 test
from tests.test_hip_moe_mxfp4 import ONE, RAGGED, BIG, GEMM_CASES, _x

pytestmark = pytest.mark.gpu

_TABLES = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda")


def _tables(E, K, I, Hd, dev):
    """(W float64 [E, N, K] = s * e4m3(q), fp8 frag codes, group scales fp32 [E, N / 16, K / 128]) of random gate_up and down experts:
    one geometry at a time, generated once and never modified."""
    from ssd_amd import quant
    from ssd_amd.hip import quant_ops as Q
    if (E, K, I, Hd) in _TABLES:
        return _TABLES[(E, K, I, Hd)]
    _TABLES.clear()
    g = torch.Generator(device=dev).manual_seed(E + K + I + Hd)
    out = ()
    for N, Kc, row_map in ((2 * I, K, quant.gate_up_row_map(2 * I).to(dev)), (Hd, I, None)):
        q = torch.randint(0, 127, (E, N, Kc), generator=g, device=dev, dtype=torch.uint8)           # 0x7F never
        q |= torch.randint(0, 2, (E, N, Kc), generator=g, device=dev, dtype=torch.uint8) << 7
        sg = torch.exp2(4.0 * torch.rand(E, N // 16, Kc // 128, generator=g, device=dev) - 9.0) \
            * (1.0 + torch.rand(E, N // 16, Kc // 128, generator=g, device=dev))                   # by PACKED group
        src = torch.arange(N, device=dev) if row_map is None else row_map.long()
        W = torch.empty(E, N, Kc, dtype=R.F64, device=dev)
        frag = torch.empty(E, N * Kc, dtype=torch.uint8, device=dev)
        for e in range(E):
            rowscale = torch.empty(N, Kc // 128, dtype=R.F64, device=dev)
            rowscale[src] = sg[e].to(R.F64).repeat_interleave(16, dim=0)                             # packed row r scales source row src[r]
            W[e] = q[e].view(quant.FP8).to(R.F64) * rowscale.repeat_interleave(128, dim=1)
            Q.fp8_rows_to_frag(q[e], frag[e], N, Kc, row_map=row_map)
        out += (W, frag.view(-1), sg.contiguous().view(-1))
    torch.cuda.synchronize()
    _TABLES[(E, K, I, Hd)] = out
    return out


def _poison_unchosen(tab, ids, E, value):
    """A copy of a table with every expert no row chose filled with `value`."""
    out = tab.clone().view(E, -1)
    chosen = torch.zeros(E, dtype=torch.bool, device=tab.device)
    chosen[ids.reshape(-1).long()] = True
    out[~chosen] = value
    return out.view(-1)


def _run(dev, shape, E, ids, x, check=True, what=""):
    """Both GEMMs for the routes ids [T, k] and rows x [T, K] -> (act, d) bf16 by entry."""
    from ssd_amd.hip import moe_ops as M
    K, I, Hd = shape
    Wgu, gq, gs, Wd, dq, ds = _tables(E, K, I, Hd, dev)
    T, k = ids.shape
    n = T * k
    assert all(len(set(r)) == k for r in ids.tolist()), "input problem: a row names an expert twice"
    offs, perm = R.group_tables(ids, E)
    xp = torch.full((T + 3, K), NAN, dtype=BF, device=dev)        # the rows past T: nobody names them
    xp[:T] = x
    act = torch.full((n + 3, I), SENT, dtype=torch.int16, device=dev)
    d = torch.full((n + 3, Hd), SENT, dtype=torch.int16, device=dev)
    M.moe_gemm_fp8b(xp, _poison_unchosen(gq, ids, E, 0x7F), _poison_unchosen(gs, ids, E, NAN), offs, perm, act, T, k, E, 2 * I, K, M.EPI_UP)
    M.moe_gemm_fp8b(act, _poison_unchosen(dq, ids, E, 0x7F), _poison_unchosen(ds, ids, E, NAN), offs, perm, d, T, k, E, Hd, I, M.EPI_DOWN)
    torch.cuda.synchronize()
    assert bool((act[n:] == SENT).all() and (d[n:] == SENT).all()), f"{what}: a write past the T * k entries"
    act_b, d_b = act[:n].view(BF), d[:n].view(BF)
    assert bool(torch.isfinite(act_b.float()).all() and torch.isfinite(d_b.float()).all()), f"{what}: an entry was not written, or poison leaked in"
    if check:
        gu64, gumag = R.grouped_exact(x, Wgu, ids, gather_tokens=True)
        R.assert_act_within_bar(act_b, gu64[:, :I], gumag[:, :I], gu64[:, I:], gumag[:, I:], f"{what} act")
        d64, dmag = R.grouped_exact(act_b, Wd, ids, gather_tokens=False)
        R.assert_within_bar(d_b, d64, dmag, f"{what} d")
    return act_b, d_b


@pytest.mark.parametrize("shape,E,k,T,kind", GEMM_CASES)
def test_gemm_chain(dev, shape, E, k, T, kind):
    ids = _routing(kind, T, k, E, dev).int()
    _run(dev, shape, E, ids, _x(T, shape[0], T + k, dev), what=f"{shape} E={E} k={k} T={T} {kind}")


@pytest.mark.parametrize("shape,E,k", [(ONE, 8, 2), (RAGGED, 8, 8), (BIG, 128, 8)])
def test_a_row_alone_and_in_a_prefill_give_equal_bits(dev, shape, E, k):
    """The accumulation order is a function of K only: token row 57 of a 130-row batch with other routes around it == that row at T = 1."""
    T, t = 130, 57
    ids = _routing("random", T, k, E, dev).int()
    x = _x(T, shape[0], 9, dev)
    act, d = _run(dev, shape, E, ids, x, check=False, what="batch")
    act1, d1 = _run(dev, shape, E, ids[t:t + 1], x[t:t + 1], check=False, what="alone")
    assert torch.equal(act[t * k:(t + 1) * k].view(torch.int16), act1.view(torch.int16)), "act bits depend on the batch"
    assert torch.equal(d[t * k:(t + 1) * k].view(torch.int16), d1.view(torch.int16)), "d bits depend on the batch"


def test_graph_capture_replays_other_routes(dev):
    """up + down captured once; replays with other routes in the same offs / perm buffers equal the eager launches by bits."""
    from ssd_amd.hip import moe_ops as M
    shape, E, k, T = RAGGED, 8, 2, 24
    K, I, Hd = shape
    _, gq, gs, _, dq, ds = _tables(E, K, I, Hd, dev)
    x = _x(T, K, 5, dev)
    offs = torch.zeros(E + 1, dtype=torch.int32, device=dev)
    perm = torch.zeros(T * k, dtype=torch.int32, device=dev)
    act = torch.zeros(T * k, I, dtype=BF, device=dev)
    d = torch.zeros(T * k, Hd, dtype=BF, device=dev)

    def block():
        M.moe_gemm_fp8b(x, gq, gs, offs, perm, act, T, k, E, 2 * I, K, M.EPI_UP)
        M.moe_gemm_fp8b(act, dq, ds, offs, perm, d, T, k, E, Hd, I, M.EPI_DOWN)

    routes = {"a": R.group_tables(_routing("random", T, k, E, dev), E), "b": R.group_tables(_routing("few", T, k, E, dev), E)}
    assert not torch.equal(routes["a"][1], routes["b"][1]), "input problem: the two routes are the same"
    eager = {}
    for name, (o, p) in routes.items():
        offs.copy_(o)
        perm.copy_(p)
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
    for name in ("b", "a", "b"):
        offs.copy_(routes[name][0])
        perm.copy_(routes[name][1])
        act.fill_(NAN)
        d.fill_(NAN)
        graph.replay()
        torch.cuda.synchronize()
        for got, want, what in zip((act, d), eager[name], ("act", "d")):
            assert torch.equal(got.view(torch.int16), want.view(torch.int16)), f"replay with routes {name}: {what} differs from the eager launch"


def test_refusals(dev):
    """Every SSD_ERR_* the header promises, before any launch (the output keeps its bits)."""
    from ssd_amd.hip import moe_ops as M
    from ssd_amd.hip.ops import _p, _stream
    SHAPE, ARG = -1, -3
    E, k, T, K, I = 8, 2, 4, 128, 128
    offs, perm = R.group_tables(_routing("few", T, k, E, dev), E)
    x, q = torch.zeros(T, K, dtype=BF, device=dev), torch.zeros(E * 2 * I * K, dtype=torch.uint8, device=dev)
    s = torch.ones(E * (2 * I // 16) * (K // 128), dtype=torch.float32, device=dev)
    act = torch.full((T * k, I), SENT, dtype=torch.int16, device=dev)
    base = dict(rows=_p(x), q=_p(q), s=_p(s), offs=_p(offs), perm=_p(perm), out=_p(act), T=T, k=k, E=E, N=2 * I, K=K, epi=M.EPI_UP)
    cases = [(dict([(n, 0)]), ARG) for n in ("rows", "q", "s", "offs", "perm", "out")] + [(dict(epi=2), ARG), (dict(epi=-1), ARG)]
    cases += [(kw, SHAPE) for kw in (dict(T=0), dict(k=0), dict(k=9), dict(E=4), dict(E=20), dict(E=512), dict(K=64), dict(K=160), dict(K=0),
                                     dict(N=32), dict(N=96), dict(N=0), dict(epi=M.EPI_DOWN, N=24), dict(epi=M.EPI_DOWN, K=K + 32),
                                     dict(T=(1 << 24) // k + 1))]
    for kw, rc in cases + [({}, 0)]:
        a = dict(base, **kw)
        assert M.load_moe_fp8b_library().ssd_moe_gemm_fp8b(*a.values(), _stream()) == rc, kw
        torch.cuda.synchronize()
        assert bool((act == SENT).all()) == (rc != 0), f"{kw}: a refused call launched (or the accepted one did not)"

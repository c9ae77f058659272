"""The grouped MXFP4 expert GEMM on the MI355X through the C ABI (csrc/moe_mxfp4.hip, include/ssd_hip_moe_mxfp4.h) against
moe_ref.grouped_exact over the float64 image of the exact dequantized weights, both epilogues chained (act into down).

Poisoning in every case: x rows past T are NaN, outputs are sentinel-filled with a sentinel tail, the code and scale tables of every
expert no row chose are 0xFF bytes (scale byte 255: any use gives inf or NaN), and the scale bytes are random per row and 32-column
block in 118..130, so a wrong byte select or another row's scale shows.  Bars: those of tests/test_hip_moe.py (1 bf16 ulp of the float64
value, differences below 2^-20 * sum|x w| exempt; the down GEMM from the kernel's OWN act)."""
import pytest
import torch

from tests import moe_ref as R
from tests import mxfp4_ref as X
from tests.test_hip_moe import _routing, SENT, NAN, BF

pytestmark = pytest.mark.gpu

_TABLES = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda")


def _tables(E, K, I, Hd, dev):
    """(W bf16 [E, N, K] = 2^(b - 127) * e2m1(q), mx4 frag codes, frag scales) of random gate_up and down experts: one geometry at a
    time, generated once and never modified."""
    from ssd_amd import quant
    from ssd_amd.hip import mx4_ops as MX
    if (E, K, I, Hd) in _TABLES:
        return _TABLES[(E, K, I, Hd)]
    _TABLES.clear()
    g = torch.Generator(device=dev).manual_seed(E + K + I + Hd)
    lut = torch.tensor(list(X.MAGS) + [-m for m in X.MAGS], dtype=torch.float32, device=dev)
    out = ()
    for N, Kc, row_map in ((2 * I, K, quant.gate_up_row_map(2 * I).to(dev)), (Hd, I, None)):
        packed = torch.randint(0, 256, (E, N, Kc // 2), generator=g, device=dev, dtype=torch.uint8)
        scale = torch.randint(118, 131, (E, N, Kc // 32), generator=g, device=dev, dtype=torch.uint8)
        W = torch.empty(E, N, Kc, dtype=BF, device=dev)
        q, s = torch.empty(E, N * Kc // 2, dtype=torch.uint8, device=dev), torch.empty(E, N * Kc // 32, dtype=torch.uint8, device=dev)
        for e in range(E):
            codes = torch.stack((packed[e] & 15, packed[e] >> 4), dim=-1).reshape(N, Kc).long()
            W[e] = (lut[codes] * torch.exp2(scale[e].float() - 127.0).repeat_interleave(32, dim=1)).to(BF)       # exact in fp32 and in bf16
            MX.mx4_rows_to_frag(packed[e], scale[e], q[e], s[e], N, Kc, row_map=row_map)
        out += (W, q.view(-1), s.view(-1))
    torch.cuda.synchronize()
    _TABLES[(E, K, I, Hd)] = out
    return out


def _ff_unchosen(tab, ids, E):
    """A copy of a byte table with every expert no row chose turned into 0xFF bytes."""
    out = tab.clone().view(E, -1)
    chosen = torch.zeros(E, dtype=torch.bool, device=tab.device)
    chosen[ids.reshape(-1).long()] = True
    out[~chosen] = 0xFF
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
    M.moe_gemm_mxfp4(xp, _ff_unchosen(gq, ids, E), _ff_unchosen(gs, ids, E), offs, perm, act, T, k, E, 2 * I, K, M.EPI_UP)
    M.moe_gemm_mxfp4(act, _ff_unchosen(dq, ids, E), _ff_unchosen(ds, ids, E), offs, perm, d, T, k, E, Hd, I, M.EPI_DOWN)
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


def _x(T, K, seed, dev):
    return torch.randn(T, K, generator=torch.Generator(device=dev).manual_seed(seed), device=dev).to(BF)


# (K_up = h, I, H): one K unit (a wave without work) | 5 and 3 units, 13 row groups in the down table | the 30B shape
ONE, RAGGED, BIG = (128, 128, 128), (640, 384, 208), (2048, 768, 2048)
GEMM_CASES = [
    (ONE, 8, 1, 1, "distinct"), (ONE, 8, 1, 33, "16_17"), (ONE, 8, 2, 130, "one"), (ONE, 8, 8, 1, "distinct"), (ONE, 8, 2, 7, "few"),
    (RAGGED, 8, 1, 1, "distinct"), (RAGGED, 8, 1, 33, "16_17"), (RAGGED, 8, 8, 130, "one"), (RAGGED, 8, 2, 7, "few"),
    (RAGGED, 128, 8, 17, "random"), (RAGGED, 128, 8, 16, "distinct"), (RAGGED, 128, 1, 130, "one"),
    (BIG, 128, 8, 1, "distinct"), (BIG, 128, 8, 8, "distinct"), (BIG, 128, 8, 130, "random"), (BIG, 128, 1, 130, "one"),
    (BIG, 128, 1, 33, "16_17"), (BIG, 128, 2, 7, "few"),
]


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
        M.moe_gemm_mxfp4(x, gq, gs, offs, perm, act, T, k, E, 2 * I, K, M.EPI_UP)
        M.moe_gemm_mxfp4(act, dq, ds, offs, perm, d, T, k, E, Hd, I, M.EPI_DOWN)

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
    x, q = torch.zeros(T, K, dtype=BF, device=dev), torch.zeros(E * 2 * I * K // 2, dtype=torch.uint8, device=dev)
    act = torch.full((T * k, I), SENT, dtype=torch.int16, device=dev)
    base = dict(rows=_p(x), q=_p(q), s=_p(q), offs=_p(offs), perm=_p(perm), out=_p(act), T=T, k=k, E=E, N=2 * I, K=K, epi=M.EPI_UP)
    cases = [(dict([(n, 0)]), ARG) for n in ("rows", "q", "s", "offs", "perm", "out")] + [(dict(epi=2), ARG), (dict(epi=-1), ARG)]
    cases += [(kw, SHAPE) for kw in (dict(T=0), dict(k=0), dict(k=9), dict(E=4), dict(E=20), dict(E=512), dict(K=64), dict(K=160), dict(K=0),
                                     dict(N=32), dict(N=96), dict(N=0), dict(epi=M.EPI_DOWN, N=24), dict(epi=M.EPI_DOWN, K=K + 32),
                                     dict(T=(1 << 24) // k + 1))]
    for kw, rc in cases + [({}, 0)]:
        a = dict(base, **kw)
        assert M.load_moe_mx4_library().ssd_moe_gemm_mxfp4(*a.values(), _stream()) == rc, kw
        torch.cuda.synchronize()
        assert bool((act == SENT).all()) == (rc != 0), f"{kw}: a refused call launched (or the accepted one did not)"

"""ssd_filter_rows (csrc/filter.hip) on the GPU against the float64 restatement in tests/filter_ref.py: every row kind of the issue in a
few launches, at vocabulary sizes around the 8-entry chunk and the 1024-thread stride (8, 1000, 1024, 1025, 3000) and at the two real
ones (128256, 151936), with ld > V and sentinels behind every row, aligned rows (16-byte loads) and unaligned ones (2-byte loads).

top_k and min_p sets must equal the reference exactly.  top_p is checked with EPS = 1e-4 on masses recomputed in float64 over the
kernel's own kept set (fp32 partial sums of at most 192 terms per thread plus __expf, with about eight-fold headroom); where the
reference's own margin is above EPS on both sides the set must equal the reference's.  Then determinism (two runs, one hipGraph
replay) and composition with ssd_sample_rows, ssd_row_lse and ssd_verify_ratio (chi-square helper and p-value bar of
tests/test_hip_stochastic.py).

top_k >= V is "off" by the semantics (the row comes back untouched); top_k = 1, top_p = 1e-6 and min_p = 1.0 keep the maximum's class."""
import numpy as np
import pytest
import torch

from tests import filter_ref as R

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
EPS = 1e-4
NEG_INF_BITS = 0xFF80
OFF = (1.0, 0, 1.0, 0.0)        # (temperature, top_k, top_p, min_p)


@pytest.fixture(scope="module")
def F():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ssd_amd.hip import filter_ops
    return filter_ops


def bits(t: torch.Tensor) -> np.ndarray:
    return t.contiguous().view(torch.int16).cpu().numpy().astype(np.int64) & 0xFFFF


def param_tensors(params, device="cuda"):
    return (torch.tensor([p[0] for p in params], dtype=torch.float32, device=device),
            torch.tensor([p[1] for p in params], dtype=torch.int32, device=device),
            torch.tensor([p[2] for p in params], dtype=torch.float32, device=device),
            torch.tensor([p[3] for p in params], dtype=torch.float32, device=device))


def launch(F, rows: torch.Tensor, V: int, params, rpp: int, offset: int = 0):
    """rows bf16 [T, ld] on the host -> (filtered rows, kept) on the host.  offset: the first row starts that many entries behind a
    16-byte boundary (an odd offset: no row of the launch can take the 16-byte loads)."""
    T, ld = rows.shape
    d = torch.zeros(T * ld + 8, dtype=BF, device="cuda")[offset:offset + T * ld].view(T, ld)
    d.copy_(rows)
    kept = torch.full((T,), -7, dtype=torch.int32, device="cuda")
    F.filter_rows(d, ld, T, V, *param_tensors(params), rpp, kept)
    torch.cuda.synchronize()
    return d.cpu(), kept.cpu()


def with_sentinels(x: torch.Tensor, ld: int) -> torch.Tensor:
    """[T, V] -> [T, ld] with +inf and NaN behind every row."""
    T, V = x.shape
    out = torch.empty(T, ld, dtype=BF)
    out[:, :V] = x
    tail = torch.tensor([float("inf"), float("nan")], dtype=BF).repeat((ld - V + 1) // 2)[:ld - V]
    out[:, V:] = tail
    return out


def check_row(xin: np.ndarray, bin_: np.ndarray, bout: np.ndarray, kept: int, prm, what: str) -> str:
    """All per-row assertions.  xin: float64 values, bin_ / bout: bf16 bit patterns before / after.  Returns how top_p was judged:
    "-" (top_p off or row untouched), "equal" (margin above EPS: the set equals the reference's) or "eps" (EPS property alone)."""
    T, k, p, mp = prm
    V = xin.shape[0]
    ref = R.filter_row(xin, T, k, p, mp)
    if not ref.touched:
        assert np.array_equal(bin_, bout), f"{what}: an untouched row changed"
        assert kept == V, f"{what}: kept={kept} for an untouched row"
        return "-"
    nan = np.isnan(xin)
    same = bin_ == bout
    dropped = ~same
    assert (bout[dropped] == NEG_INF_BITS).all(), f"{what}: a changed entry is not -inf"
    assert not (same & nan).any(), f"{what}: a NaN survived"
    was_ninf = bin_ == NEG_INF_BITS                       # kept or dropped, such an entry looks the same afterwards
    got = same & ~nan & ~was_ninf                         # the kernel's kept set, up to entries that were -inf before
    assert got.sum() <= kept <= got.sum() + was_ninf.sum(), f"{what}: kept={kept}, counted {got.sum()} (+{was_ninf.sum()} -inf)"
    assert got.any(), f"{what}: the row was emptied"
    out_of = ~got & ~nan
    if out_of.any():                                      # an upper set of the row's values
        assert xin[got].min() > xin[out_of].max(), f"{what}: not an upper set"
    assert got[xin == np.nanmax(xin)].all(), f"{what}: the maximum's class was dropped"
    e, mx = ref.e, np.nanmax(xin)
    if mp > 0:                                            # precondition of exact min_p equality
        rest = e[~nan & (xin != mx)]
        assert (np.abs(rest - R.f32(mp)) > EPS * R.f32(mp)).all(), f"{what}: an e_i lies within {EPS} of min_p (choose another)"
    want = ref.keep & ~was_ninf
    if R.f32(p) >= 1.0:                                   # top_k and min_p: exact
        assert np.array_equal(got, want), f"{what}: kept {got.sum()}, reference {want.sum()}"
        assert kept == ref.keep.sum(), what
        return "-"
    if ref.p_margin > EPS:
        assert np.array_equal(got, want), f"{what}: kept {got.sum()}, reference {want.sum()} at margin {ref.p_margin:.3g}"
        assert kept == ref.keep.sum(), what
        return "equal"
    # EPS property on the kernel's own set (only where min_p does not cut into the nucleus)
    in_k = ref.in_k & ~was_ninf
    assert mp == 0 or np.array_equal(ref.keep, R.filter_row(xin, T, k, p, 0.0).keep), \
        f"{what}: margin {ref.p_margin:.3g} <= EPS on a row where min_p binds (choose another)"
    assert not (got & ~in_k).any(), f"{what}: kept something outside the top-k set"
    zk = e[ref.in_k].sum()
    mass = e[got].sum()
    lowest = got & (xin == xin[got].min())
    print(f"{what}: eps-only, margin {ref.p_margin:.3g}, kept {got.sum()} vs reference {want.sum()}, "
          f"mass/target {mass / (R.f32(p) * zk):.7f}, without lowest class {(mass - e[lowest].sum()) / (R.f32(p) * zk):.7f}")
    assert mass >= R.f32(p) * zk * (1 - EPS), what
    assert mass - e[lowest].sum() < R.f32(p) * zk * (1 + EPS), what
    return "eps"


def check_launch(inp: torch.Tensor, out: torch.Tensor, kept: torch.Tensor, V: int, params, rpp: int, what: str):
    bi, bo = bits(inp), bits(out)
    assert np.array_equal(bi[:, V:], bo[:, V:]), f"{what}: entries in [V, ld) were touched"
    xin = inp[:, :V].float().numpy().astype(np.float64)
    return [check_row(xin[r], bi[r, :V], bo[r, :V], int(kept[r]), params[r // rpp], f"{what} row {r} {params[r // rpp]}")
            for r in range(inp.shape[0])]


# ---------------------------------------------------------------------------------------------------------------------
# row kinds
# ---------------------------------------------------------------------------------------------------------------------
def make_row(kind: str, V: int, g: torch.Generator, k: int = 0) -> torch.Tensor:
    x = (torch.randn(V, generator=g) * 2.0).to(BF)
    if kind == "flat":
        x = (torch.randn(V, generator=g) * 0.3).to(BF)
    elif kind == "equal":
        x = torch.full((V,), 1.5, dtype=BF)
    elif kind == "tie":                 # the k-th and the (k+1)-th largest are one value
        order = torch.argsort(x.float(), descending=True, stable=True)
        x[order[k]] = x[order[k - 1]]
    elif kind == "neginf":
        x[torch.randperm(V, generator=g)[:V // 4]] = float("-inf")
    elif kind == "nan":
        x[torch.randperm(V, generator=g)[:max(1, V // 50)]] = float("nan")
    elif kind == "allnan":
        x = torch.full((V,), float("nan"), dtype=BF)
    elif kind == "zeros":               # -0.0 and +0.0 are one value
        x[: V // 2] = 0.0
        x[V // 4: V // 2] = -0.0
    else:
        assert kind == "rand"
    return x


def row_plan(V: int):
    """24 (row kind, parameters) pairs: each filter alone, all together, the degenerate settings, the special rows."""
    k = max(2, min(40, V // 4))
    return [("rand", OFF), ("rand", (0.0, k, 0.5, 0.1)), ("rand", (0.8, k, 1.0, 0.0)), ("rand", (0.7, 0, 0.9, 0.0)),
            ("rand", (1.0, 0, 1.0, 0.05)), ("rand", (0.9, k + 10, 0.9, 0.02)), ("rand", (1.0, 1, 1.0, 0.0)), ("rand", (1.0, V, 1.0, 0.0)),
            ("rand", (1.0, V + 7, 1.0, 0.0)), ("rand", (1.0, 0, 1e-6, 0.0)), ("rand", (1.0, 0, 1.0, 1.0)), ("equal", (0.7, 3, 0.5, 0.5)),
            ("tie", (1.0, k, 1.0, 0.0)), ("tie", (1.0, k, 0.999, 0.0)), ("neginf", (0.8, k, 1.0, 0.0)), ("neginf", (0.8, 0, 0.9, 0.0)),
            ("neginf", (0.8, V - 2, 1.0, 0.03)), ("nan", (0.8, k, 1.0, 0.0)), ("nan", (0.9, k + 5, 0.8, 0.01)), ("allnan", (0.8, k, 0.9, 0.1)),
            ("flat", (1.0, 0, 0.5, 0.0)), ("flat", (1.3, V // 2, 1.0, 0.0)), ("zeros", (1.0, V // 3, 1.0, 0.0)), ("rand", (2.0, 0, 0.95, 0.0))]


@pytest.mark.parametrize("V,ld", [(1000, 1003), (1024, 1032), (1025, 1040), (3000, 3001)])
def test_every_row_kind_in_one_launch_of_24_rows(F, V, ld):
    g = torch.Generator().manual_seed(V)
    plan = row_plan(V)
    x = torch.stack([make_row(kind, V, g, prm[1]) for kind, prm in plan])
    inp = with_sentinels(x, ld)
    params = [prm for _, prm in plan]
    out, kept = launch(F, inp, V, params, 1)
    how = check_launch(inp, out, kept, V, params, 1, f"V={V}")
    assert how.count("eps") <= 1, how


@pytest.mark.parametrize("T", [3, 24])
def test_one_parameter_set_per_three_rows(F, T):
    V, ld, rpp = 1025, 1027, 3
    g = torch.Generator().manual_seed(T)
    params = [(0.9, 30, 0.9, 0.01), OFF, (0.0, 5, 0.5, 0.5), (1.0, 7, 1.0, 0.0), (0.6, 0, 0.8, 0.0), (1.0, 0, 1.0, 0.1),
              (1.2, 100, 0.95, 0.0), (0.8, 1, 1.0, 0.0)][:T // rpp]
    x = torch.stack([make_row("rand", V, g) for _ in range(T)])
    inp = with_sentinels(x, ld)
    out, kept = launch(F, inp, V, params, rpp)
    check_launch(inp, out, kept, V, params, rpp, f"T={T} rows_per_param=3")


def test_hand_made_rows_of_eight(F):
    """Probabilities 1/2, 1/4, ... 1/128, 1/128 (logits 0, -1, ... in units of ln 2): top_p = 0.7 keeps exactly two."""
    T = 1.0 / np.log(2.0)
    base = torch.tensor([0.0, -1, -2, -3, -4, -5, -6, -6], dtype=BF)
    perm = torch.tensor([3, 0, 7, 1, 5, 2, 6, 4])
    x = torch.stack([base, base[perm], base, base, base[perm], base])
    params = [(T, 0, 0.7, 0.0), (T, 0, 0.7, 0.0), (T, 3, 1.0, 0.0), (T, 0, 1.0, 0.1), (T, 8, 0.95, 0.0), (T, 7, 1.0, 0.0)]
    inp = with_sentinels(x, 11)
    out, kept = launch(F, inp, 8, params, 1)
    check_launch(inp, out, kept, 8, params, 1, "V=8")
    # 0.7 -> {1/2, 1/4}; top_k 3; min_p 0.1 of the largest -> 1/2 .. 1/8 (1/16 = 0.0625 < 0.1); 0.95 -> 1/2 .. 1/32 (0.96875);
    # top_k 7 meets the tie at the 7th / 8th place and keeps all eight
    assert kept.tolist() == [2, 2, 3, 4, 5, 8]
    assert (out[1, :8].float() > float("-inf")).nonzero().flatten().tolist() == [1, 3]


LARGE = [(128256, 128264, [("rand", 2.0, (0.7, 0, 0.9, 0.0)), ("rand", 0.3, (1.0, 0, 0.5, 0.0)), ("rand", 2.0, (1.0, 50, 0.95, 0.0)),
                           ("rand", 2.0, (0.8, 40, 0.9, 0.02))]),
         (151936, 151939, [("rand", 3.0, (1.0, 0, 0.9, 0.0))])]


@pytest.fixture(scope="module")
def large_rows():
    """The real vocabularies: seeded rows, built once (the reference sorts 150 000 float64 values per row)."""
    cases = []
    for V, ld, rows in LARGE:
        g = torch.Generator().manual_seed(V)
        x = torch.stack([(torch.randn(V, generator=g) * sigma).to(BF) for _, sigma, _ in rows])
        cases.append((V, ld, with_sentinels(x, ld), [prm for _, _, prm in rows]))
    g = torch.Generator().manual_seed(3000)
    cases.append((3000, 3000 + 8, with_sentinels((torch.randn(1, 3000, generator=g) * 4.0).to(BF), 3008), [(0.6, 0, 0.8, 0.0)]))
    return cases


def test_real_vocabularies_and_the_issue_s_random_cases(F, large_rows):
    how = []
    for V, ld, inp, params in large_rows:
        out, kept = launch(F, inp, V, params, 1, offset=1 if V == 151936 else 0)
        how += check_launch(inp, out, kept, V, params, 1, f"V={V}")
    print("top_p judged by:", how)
    assert how.count("eps") * 5 <= len(how), how          # at most one random-row case in five on the EPS property alone


def test_two_runs_and_a_graph_replay_are_bit_equal(F, large_rows):
    from ssd_amd.utils.graphs import capture
    V, ld, inp, params = large_rows[0]
    T = inp.shape[0]
    prm = param_tensors(params)
    a, ka = launch(F, inp, V, params, 1)
    b, kb = launch(F, inp, V, params, 1)
    assert np.array_equal(bits(a), bits(b)) and torch.equal(ka, kb)
    static = inp.cuda().contiguous()
    kept = torch.zeros(T, dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with capture(graph, stream=stream):
        F.filter_rows(static, ld, T, V, *prm, 1, kept)
    static.copy_(inp)                   # the graph replays on fresh rows
    kept.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(bits(static.cpu()), bits(a)) and torch.equal(kept.cpu(), ka)
    # fresh parameter values without a new capture: everything off -> untouched
    static.copy_(inp)
    prm[1].zero_()
    prm[2].fill_(1.0)
    prm[3].zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(bits(static.cpu()), bits(inp)) and kept.cpu().tolist() == [V] * T


def test_refusals(F):
    from ssd_amd.hip.lib import SsdHipError
    x = torch.zeros(2, 16, dtype=BF, device="cuda")
    t, k, p, m = param_tensors([OFF, OFF])
    for args in [(x, 16, 0, 16, t, k, p, m, 1), (x, 16, 2, 0, t, k, p, m, 1), (x, 16, 2, 16, t, k, p, m, 0), (x, 8, 2, 16, t, k, p, m, 1),
                 (x, F.MAX_V + 8, 1, F.MAX_V + 8, t, k, p, m, 1), (None, 16, 2, 16, t, k, p, m, 1), (x, 16, 2, 16, None, k, p, m, 1),
                 (x, 16, 2, 16, t, None, p, m, 1), (x, 16, 2, 16, t, k, None, m, 1), (x, 16, 2, 16, t, k, p, None, 1)]:
        with pytest.raises(SsdHipError, match="ssd_filter_rows"):
            F.filter_rows(*args)
    F.filter_rows(x, 16, 2, 16, t, k, p, m, 1)          # kept is optional
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# composition with the samplers
# ---------------------------------------------------------------------------------------------------------------------
def chi2_ok(counts: torch.Tensor, probs: torch.Tensor, what: str):
    """tests/test_hip_stochastic.py chi2_ok: same pooling of thin bins, same p > 1e-4 bar."""
    from scipy.stats import chisquare
    n = counts.sum().item()
    keep = probs * n >= 5
    obs = torch.cat([counts[keep].double(), counts[~keep].double().sum().view(1)])
    exp = torch.cat([(probs[keep] * n).double(), (probs[~keep] * n).double().sum().view(1)])
    if exp[-1] < 1e-9:
        obs, exp = obs[:-1], exp[:-1]
    exp = exp * obs.sum() / exp.sum()
    stat, p = chisquare(obs.numpy(), exp.numpy())
    print(f"{what}: chi2={stat:.1f} p={p:.4f} bins={len(obs)} n={n}")
    assert p > 1e-4, f"{what}: chi-square p={p}"


def rng(seed=1):
    return torch.tensor([seed], dtype=torch.int64, device="cuda")


@pytest.mark.parametrize("V,N,prm", [(64, 6000, (0.8, 12, 0.85, 0.02)), (3000, 4000, (0.9, 40, 0.9, 0.0))])
def test_filter_then_sample_rows_and_row_lse(F, V, N, prm):
    from ssd_amd.hip import ops as H
    g = torch.Generator().manual_seed(V + 1)
    x = (torch.randn(V, generator=g) * 1.5).to(BF)
    ref = R.filter_row(x.float().numpy(), *prm)
    assert ref.p_margin > EPS
    probs = torch.from_numpy(R.renormalised(ref))
    rows = x.unsqueeze(0).repeat(N, 1).cuda().contiguous()
    temps, ks, ps, ms = param_tensors([prm])
    F.filter_rows(rows, V, N, V, temps, ks, ps, ms, N)          # one parameter set for all N rows
    out = torch.zeros(N, dtype=torch.int64, device="cuda")
    H.sample_rows(rows, V, N, V, temps, N, rng(3), 11, out)
    lse = torch.zeros(N, device="cuda")
    H.row_lse(rows, V, N, V, temps, N, lse)
    counts = torch.bincount(out.cpu(), minlength=V)
    assert counts[torch.from_numpy(~ref.keep)].sum() == 0, "a token outside the kept set was drawn"
    chi2_ok(counts, probs, f"filter + sample_rows V={V}")
    # lse = log of the kept mass: log(sum over kept of exp(s - m)) + m
    m = x.float().max().item() / R.f32(prm[0])
    want = np.log(ref.e[ref.keep].sum()) + m
    assert (lse.cpu() - want).abs().max().item() < 2e-3          # tests/test_hip_stochastic.py test_row_lse's tolerance


def test_filter_p_and_q_then_verify_ratio_emits_the_filtered_p(F):
    """Speculative sampling on truncated distributions: one draft position (K = 1), x ~ filtered q drawn by ssd_sample_rows, then
    ssd_verify_ratio on filtered p and q.  The emitted token (x if accepted, the recovery otherwise) is distributed as filtered p."""
    from ssd_amd.hip import ops as H
    V, N, K = 48, 30000, 1
    g = torch.Generator().manual_seed(5)
    lp1 = (torch.randn(K + 1, V, generator=g) * 1.2).to(BF)
    lq1 = (lp1[:K].float() + torch.randn(K, V, generator=g) * 0.8).to(BF)
    prm_t, prm_q = (0.9, 12, 0.9, 0.0), (1.1, 12, 0.9, 0.0)          # the engine filters p and q with the same top_k / top_p / min_p
    ref_p = R.filter_row(lp1[0].float().numpy(), *prm_t)
    assert ref_p.p_margin > EPS and R.filter_row(lq1[0].float().numpy(), *prm_q).p_margin > EPS
    lp = lp1.unsqueeze(0).repeat(N, 1, 1).view(N * (K + 1), V).cuda().contiguous()
    lq = lq1.unsqueeze(0).repeat(N, 1, 1).view(N * K, V).cuda().contiguous()
    tt, ks, ps, ms = param_tensors([prm_t] * N)
    tq = torch.full((N,), prm_q[0], device="cuda")
    F.filter_rows(lp, V, N * (K + 1), V, tt, ks, ps, ms, K + 1)
    F.filter_rows(lq, V, N * K, V, tq, ks, ps, ms, K)
    x = torch.zeros(N, dtype=torch.int64, device="cuda")
    H.sample_rows(lq, V, N, V, tq, 1, rng(7), 5, x)
    spec = torch.stack([torch.full((N,), 7, dtype=torch.int64, device="cuda"), x], dim=1).contiguous()
    preds = torch.zeros(N * (K + 1), dtype=torch.int64, device="cuda")
    H.argmax_rows(lp, V, N * (K + 1), V, preds)                      # (rows of 48 * 2 bytes are 16-byte aligned, as it needs)
    lse_p = torch.zeros(N * (K + 1), device="cuda")
    lse_q = torch.zeros(N * K, device="cuda")
    H.row_lse(lp, V, N * (K + 1), V, tt, K + 1, lse_p)
    H.row_lse(lq, V, N * K, V, tq, K, lse_q)
    acc = torch.zeros(N, dtype=torch.int32, device="cuda")
    rec = torch.zeros(N, dtype=torch.int64, device="cuda")
    H.verify_ratio(lp, V, lq, V, V, N, K, spec, preds, lse_p, lse_q, tt, tq, torch.ones(N, dtype=torch.int32, device="cuda"), rng(9), 2,
                   acc, rec, None, None)
    torch.cuda.synchronize()
    acc, rec, x = acc.cpu(), rec.cpu(), x.cpu()
    emitted = torch.where(acc >= 1, x, rec)
    assert 0 < (acc >= 1).sum().item() < N                         # both the accept and the reject branch
    counts = torch.bincount(emitted, minlength=V)
    assert counts[torch.from_numpy(~ref_p.keep)].sum() == 0, "a token outside the filtered p was emitted"
    chi2_ok(counts, torch.from_numpy(R.renormalised(ref_p)), "emitted token ~ filtered p")

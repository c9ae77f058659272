"""GPU checks of the per-request seed kernels (csrc/seeded.hip, include/ssd_hip_seed.h).

Everything deterministic is exact: the device stream against tests/seed_ref.py by bits, unseeded rows against ssd_sample_rows /
ssd_verify_ratio by bits, a seeded row's token under every change of batch, slot, rng word, salt and row stride, a seeded sequence's
accepted length against its own acceptance probabilities and uniforms.  The draws are distributional: chi-square at p > 1e-4
(chi2_ok of tests/test_hip_stochastic.py, copied) over seeds at one position and over positions under one seed.

Vocabularies: 96 (one slice), 4096 (the slice edge), 4104 (a ragged tail), 12296 (three slices), 128256 (the real one); row strides
that keep the rows 16-byte aligned (vector loads) and strides that do not (element loads)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ops as O
from tests import seed_ref as R

BF = torch.bfloat16
I64 = torch.int64
VOCABS = [(96, 8), (96, 3), (4096, 8), (4104, 8), (4104, 3), (12296, 8), (12296, 5), (4101, 0), (128256, 8)]      # (V, ld - V)


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ssd_amd.hip import ops
    return ops


@pytest.fixture(scope="module")
def S(H):
    from ssd_amd.hip import seed_ops
    return seed_ops


def dev(t):
    return t.cuda().contiguous()


def word(v=1):
    return torch.tensor([v], dtype=I64, device="cuda")


def chi2_ok(counts: torch.Tensor, probs: torch.Tensor, what: str):
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


def draw(S, lg, ld, T, V, temps, rpt, st, salt, seeds, rps, pos, purpose, **kw):
    """ssd_sample_rows_seeded over device tensors -> tokens on the host."""
    out = torch.full((T,), -7, dtype=I64, device="cuda")
    ws = torch.zeros(S.sample_seeded_ws_bytes(T, V) // 8, dtype=I64, device="cuda")
    S.sample_rows_seeded(lg, ld, T, V, temps, rpt, st, salt, out, seeds, rps, pos, purpose, ws, **kw)
    return out.cpu()


def random_seeds(n: int, salt: int) -> torch.Tensor:
    """n seeds from all of [0, 2^63)."""
    return torch.from_numpy(np.random.default_rng(salt).integers(0, 2 ** 63, n, dtype=np.int64))


def padded(x: torch.Tensor, ld: int, fill=float("nan")) -> torch.Tensor:
    """[T][V] -> device [T][ld] with `fill` past V (alternating with +inf: neither may ever be read into a result)."""
    T, V = x.shape
    buf = torch.full((T, ld), fill, dtype=BF)
    buf[:, V::2] = float("inf")
    buf[:, :V] = x
    return dev(buf)


# ---------------------------------------------------------------------------------------------------------------------
# the stream
# ---------------------------------------------------------------------------------------------------------------------
def test_device_stream_equals_the_definition_by_bits(S):
    g = np.random.default_rng(0)
    rows, n = 64, 512
    seeds = np.array([0, 1, 2 ** 63 - 1] * 5 + [-1] + g.integers(0, 2 ** 63, rows - 16).tolist(), dtype=np.int64)
    pos = np.array([0, 255, 256, 8191, 2 ** 31] * 12 + [7, 8, 9, 10], dtype=np.int64)
    d_seed, d_pos = dev(torch.from_numpy(seeds)), dev(torch.from_numpy(pos))
    for purpose in (S.DRAFT, S.TARGET, S.ACCEPT):
        for idx0 in (0, 128256 - n, 2 ** 32 - n):
            out = torch.zeros(rows, n, dtype=torch.float32, device="cuda")
            S.seeded_uniforms(d_seed, d_pos, rows, purpose, idx0, n, out)
            got = out.cpu().numpy()
            # (the kernels take the input token's position: the key's position is one more)
            want = R.uniform(seeds.astype(np.uint64)[:, None], purpose, (pos + 1).astype(np.uint64)[:, None],
                             (idx0 + np.arange(n)).astype(np.uint64)[None, :])
            on = seeds >= 0
            assert np.array_equal(got[on].view(np.int32), want[on].view(np.int32)), (purpose, idx0)
            assert np.isnan(got[~on]).all() and (~on).sum() == 1
    # the first known answer, through the device: (seed 0, DRAFT, position 0, index 0) = input position -1
    one = torch.zeros(1, 1, dtype=torch.float32, device="cuda")
    S.seeded_uniforms(dev(torch.tensor([0], dtype=I64)), dev(torch.tensor([-1], dtype=I64)), 1, S.DRAFT, 0, 1, one)
    assert float(one.item()).hex() == "0x1.1c97d40000000p-3"


# ---------------------------------------------------------------------------------------------------------------------
# unseeded rows are ssd_sample_rows
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,pad", VOCABS)
def test_unseeded_rows_equal_the_legacy_sampler(H, S, V, pad):
    torch.manual_seed(V + pad)
    T, ld, rpt = 300, V + pad, 3
    x = (torch.randn(T, V) * 2).to(BF)
    x[4] = float("nan")                 # nothing comparable: token 0, unseeded (row 4) and seeded (row 5)
    x[5] = float("nan")
    x[6, 3] = float("nan")              # a NaN entry never wins
    x[8, V - 1] = 30.0                  # the last entry of the ragged tail wins
    x[9, 5] = x[9, V - 2] = 25.0        # (temperature 0 below) a tie across slices: the lower index
    lg = padded(x, ld)
    temps = torch.full((T // rpt,), 0.8)
    temps[3::4] = 0.0                   # rows 9..11, 21..23, ...: argmax, seeded or not
    temps[1] = 1.7
    d_temps = dev(temps)
    seeds = torch.arange(T, dtype=I64) * 7919 + 1
    seeds[0::2] = -1                    # alternate rows draw from the engine's stream
    d_seeds, d_pos = dev(seeds), dev(torch.arange(T, dtype=I64) + 40)
    top = torch.zeros(T, 4, dtype=torch.int32, device="cuda")
    H.topk_rows(lg, ld, T, V, 4, top)
    for st, salt, boost in ((word(3), 11, {}), (word(2 ** 40 + 5), 4, dict(boost_idx=top, boost_k=4, boost_x=0.4)),
                            (word(77), 2 ** 24 + 3, {})):
        legacy, legacy2 = torch.zeros(T, dtype=I64, device="cuda"), torch.zeros(T, dtype=I64, device="cuda")
        H.sample_rows(lg, ld, T, V, d_temps, rpt, st, salt, legacy, out2=legacy2, **boost)
        out2 = torch.full((T,), -3, dtype=I64, device="cuda")
        got = draw(S, lg, ld, T, V, d_temps, rpt, st, salt, d_seeds, 1, d_pos, S.TARGET, out2=out2, **boost)
        legacy = legacy.cpu()
        assert torch.equal(got, out2.cpu()) and torch.equal(legacy, legacy2.cpu())
        off = seeds < 0
        assert torch.equal(got[off], legacy[off])                       # bit for bit, rows >= 256 included
        cold = temps.repeat_interleave(rpt) == 0
        assert torch.equal(got[cold], legacy[cold]) and cold.sum() > 60 # temperature 0: the argmax, whatever the seed
        assert got[4] == 0 and got[5] == 0 and got[9] == 5 and got[6] != 3
        assert ((got >= 0) & (got < V)).all()
        hot = ~off & ~cold
        hot[5] = False
        assert (got[hot] != legacy[hot]).float().mean().item() > 0.5    # the seeded rows do draw from another stream
    # all rows unseeded, one seed per 3 rows: the whole launch is the legacy sampler
    none = dev(torch.full((T // 3,), -1, dtype=I64))
    legacy = torch.zeros(T, dtype=I64, device="cuda")
    H.sample_rows(lg, ld, T, V, d_temps, rpt, word(9), 1, legacy)
    assert torch.equal(draw(S, lg, ld, T, V, d_temps, rpt, word(9), 1, none, 3, d_pos, S.DRAFT), legacy.cpu())


# ---------------------------------------------------------------------------------------------------------------------
# a seeded row depends on nothing but (seed, position, purpose) and its own logits
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,pad", VOCABS)
def test_seeded_token_is_invariant(H, S, V, pad):
    torch.manual_seed(1000 + V + pad)
    T, ld = 48, V + pad
    x = (torch.randn(T, V) * 1.5).to(BF)
    temps = dev(torch.full((T,), 0.9))
    seeds = torch.randint(0, 2 ** 62, (T,), dtype=I64)
    pos = torch.randint(0, 8192, (T,), dtype=I64)
    lg = padded(x, ld)
    base = draw(S, lg, ld, T, V, temps, 1, word(1), 1, dev(seeds), 1, dev(pos), S.TARGET)
    # permuted rows
    perm = torch.randperm(T)
    got = draw(S, padded(x[perm], ld), ld, T, V, temps, 1, word(1), 1, dev(seeds[perm]), 1, dev(pos[perm]), S.TARGET)
    assert torch.equal(got, base[perm])
    # the row alone
    for r in (0, 17, T - 1):
        alone = draw(S, padded(x[r:r + 1], ld), ld, 1, V, temps, 1, word(1), 1, dev(seeds[r:r + 1]), 1, dev(pos[r:r + 1]), S.TARGET)
        assert alone.tolist() == [int(base[r])]
    # another rng word, another salt, the word moved on between launches
    st = word(987654321)
    assert torch.equal(draw(S, lg, ld, T, V, temps, 1, st, 99, dev(seeds), 1, dev(pos), S.TARGET), base)
    H.rng_advance(st)
    assert torch.equal(draw(S, lg, ld, T, V, temps, 1, st, 2 ** 25, dev(seeds), 1, dev(pos), S.TARGET), base)
    # a longer row stride (and with it another alignment of the rows)
    for more in (8, 13):
        assert torch.equal(draw(S, padded(x, ld + more), ld + more, T, V, temps, 1, word(1), 1, dev(seeds), 1, dev(pos), S.TARGET), base)
    # a seed shared by 4 consecutive rows at 4 positions = the same seeds row by row
    shared = seeds[::4].repeat_interleave(4)
    a = draw(S, lg, ld, T, V, temps, 1, word(1), 1, dev(seeds[::4].clone()), 4, dev(pos), S.TARGET)
    b = draw(S, lg, ld, T, V, temps, 1, word(1), 1, dev(shared), 1, dev(pos), S.TARGET)
    assert torch.equal(a, b)


def test_seed_position_and_purpose_each_change_the_draw(S):
    torch.manual_seed(5)
    T, V = 2000, 4104
    x = (torch.randn(T, V) * 0.01).to(BF)               # near-flat: the noise decides
    lg, temps = dev(x), dev(torch.full((T,), 1.0))
    seeds, pos = torch.arange(T, dtype=I64) + 10, torch.full((T,), 100, dtype=I64)
    base = draw(S, lg, V, T, V, temps, 1, word(1), 1, dev(seeds), 1, dev(pos), S.TARGET)
    for what, got in (("seed", draw(S, lg, V, T, V, temps, 1, word(1), 1, dev(seeds + T), 1, dev(pos), S.TARGET)),
                      ("position", draw(S, lg, V, T, V, temps, 1, word(1), 1, dev(seeds), 1, dev(pos + 1), S.TARGET)),
                      ("purpose", draw(S, lg, V, T, V, temps, 1, word(1), 1, dev(seeds), 1, dev(pos), S.DRAFT))):
        changed = (got != base).float().mean().item()
        print(f"changing the {what} changes {changed:.3f} of the tokens")
        assert changed > 0.5, what
    assert len(torch.unique(base)) > T // 2               # and the rows do not share their noise


# ---------------------------------------------------------------------------------------------------------------------
# distribution (the fixed row and temperature of test_sample_rows_distribution_and_greedy)
# ---------------------------------------------------------------------------------------------------------------------
def test_seeded_draws_follow_the_softmax(H, S):
    torch.manual_seed(0)
    V, N, T = 96, 40000, 0.8
    logits = (torch.randn(V) * 1.5).to(BF)
    rows = dev(logits.unsqueeze(0).repeat(N, 1))
    temps = dev(torch.full((N,), T))
    probs = torch.softmax(logits.float() / T, dim=-1)
    many, one = torch.arange(N, dtype=I64), torch.zeros(N, dtype=I64)
    out = draw(S, rows, V, N, V, temps, 1, word(3), 11, dev(random_seeds(N, 1)), 1, dev(one + 17), S.TARGET)
    chi2_ok(torch.bincount(out, minlength=V), probs, "40000 seeds at one position")
    out = draw(S, rows, V, N, V, temps, 1, word(3), 11, dev(one + 123456789), 1, dev(many), S.TARGET)
    chi2_ok(torch.bincount(out, minlength=V), probs, "40000 positions under one seed")
    out = draw(S, rows, V, N, V, temps, 1, word(3), 11, dev(one + 5), 1, dev(many), S.DRAFT)
    chi2_ok(torch.bincount(out, minlength=V), probs, "40000 positions under one seed, draft purpose")
    # sampler_x boost rows: the rescaled distribution of oracle.ops
    F, X = 3, 0.4
    top = torch.zeros(N, F + 1, dtype=torch.int32, device="cuda")
    H.topk_rows(rows, V, N, V, F + 1, top)
    want = O.sampler_x_rescale(probs.unsqueeze(0), X, F)[0]
    out = draw(S, rows, V, N, V, temps, 1, word(3), 11, dev(many + 1), 1, dev(one + 3), S.DRAFT, boost_idx=top, boost_k=F + 1, boost_x=X)
    chi2_ok(torch.bincount(out, minlength=V), want, "seeds with sampler_x")
    out = draw(S, rows, V, N, V, temps, 1, word(3), 11, dev(one + 99), 1, dev(many), S.DRAFT, boost_idx=top, boost_k=F + 1, boost_x=X)
    chi2_ok(torch.bincount(out, minlength=V), want, "positions with sampler_x")


# ---------------------------------------------------------------------------------------------------------------------
# ratio verification
# ---------------------------------------------------------------------------------------------------------------------
def run_verify(H, S, lp, lq, spec, tt, tq, ratio, seeds=None, pos=None, st=5, salt=2):
    """seeds None: ssd_verify_ratio; else ssd_verify_ratio_seeded.  -> (accept_len, recovery, packed, accept_prob) on the host."""
    B, Kp1, V = lp.shape
    K = Kp1 - 1
    d_lp, d_lq = dev(lp.reshape(B * Kp1, V)), dev(lq.reshape(B * K, V))
    preds = torch.zeros(B * Kp1, dtype=I64, device="cuda")
    H.argmax_rows(d_lp, V, B * Kp1, V, preds)
    lse_p, lse_q = torch.zeros(B * Kp1, device="cuda"), torch.zeros(B * K, device="cuda")
    H.row_lse(d_lp, V, B * Kp1, V, dev(tt), Kp1, lse_p)
    H.row_lse(d_lq, V, B * K, V, dev(tq), K, lse_q)
    acc = torch.zeros(B, dtype=torch.int32, device="cuda")
    rec = torch.zeros(B, dtype=I64, device="cuda")
    packed = torch.zeros(B, K + 3, dtype=I64, device="cuda")
    ap = torch.zeros(B, K, device="cuda")
    args = (d_lp, V, d_lq, V, V, B, K, dev(spec), preds, lse_p, lse_q, dev(tt), dev(tq), dev(ratio.to(torch.int32)), word(st), salt, acc, rec)
    if seeds is None:
        H.verify_ratio(*args, packed, ap)
    else:
        S.verify_ratio_seeded(*args, dev(seeds), dev(pos), packed=packed, accept_prob=ap)
    torch.cuda.synchronize()
    return acc.cpu(), rec.cpu(), packed.cpu(), ap.cpu()


def mixed_batch(B=256, K=3, V=48):
    """Every combination of (seeded, sampling target, sampling draft, ratio row), 16 sequences each in turn."""
    torch.manual_seed(11)
    b = torch.arange(B)
    lp = (torch.randn(B, K + 1, V) * 1.2).to(BF)
    lq = (lp[:, :K].float() + torch.randn(B, K, V) * 0.8).to(BF)
    tt = torch.where(b & 2 > 0, torch.tensor(0.9), torch.tensor(0.0))
    tq = torch.where(b & 4 > 0, torch.tensor(1.1), torch.tensor(0.0))
    ratio = b & 8 > 0
    seeds = torch.where(b & 1 > 0, b.to(I64) * 104729 + 3, torch.tensor(-1, dtype=I64))
    x = torch.where(torch.rand(B, K) < 0.5, lq.float().argmax(-1), lp[:, :K].float().argmax(-1))     # the draft's or the target's mode
    spec = torch.cat([torch.randint(0, V, (B, 1)), x], dim=1).to(I64)
    pos = (torch.randint(0, 4000, (B, 1)) + torch.arange(K + 1)).to(I64)
    return lp, lq, spec, tt, tq, ratio, seeds, pos


def test_verify_deterministic_parts_and_the_acceptance_rule(H, S):
    lp, lq, spec, tt, tq, ratio, seeds, pos = mixed_batch()
    B, K = spec.shape[0], spec.shape[1] - 1
    acc0, rec0, packed0, ap0 = run_verify(H, S, lp, lq, spec, tt, tq, ratio)
    acc, rec, packed, ap = run_verify(H, S, lp, lq, spec, tt, tq, ratio, seeds, pos)
    assert torch.equal(ap.view(torch.int32), ap0.view(torch.int32))                       # accept_prob: every sequence, by bits
    off = seeds < 0
    assert torch.equal(acc[off], acc0[off]) and torch.equal(rec[off], rec0[off]) and torch.equal(packed[off], packed0[off])
    greedy = (tt == 0) & (tq == 0)
    assert torch.equal(acc[greedy], acc0[greedy]) and torch.equal(rec[greedy], rec0[greedy])
    # not a ratio row: greedy acceptance (deterministic); its recovery token is a draw from p unless the target is greedy
    plain = ~ratio
    assert torch.equal(acc[plain], acc0[plain]) and torch.equal(rec[plain & (tt == 0)], rec0[plain & (tt == 0)])
    cold = tt == 0                                                                        # a greedy target recovers with the argmax of row n
    preds = lp.float().argmax(-1)
    assert all(int(rec[b]) == int(preds[b, int(acc[b])]) for b in range(B) if cold[b])
    # the packed row agrees with accept_len / recovery
    assert torch.equal(packed[:, 0], acc.long()) and torch.equal(packed[:, 1], rec) and torch.equal(packed[:, 2:], spec)
    # seeded ratio sequences: accept_len = the first i with !(u_i <= accept_prob[b][i]), u_i the ACCEPT uniform at the input's position
    u = torch.zeros(B * (K + 1), 1, device="cuda")
    S.seeded_uniforms(dev(seeds.repeat_interleave(K + 1)), dev(pos.reshape(-1)), B * (K + 1), S.ACCEPT, 0, 1, u)
    u = u.cpu().view(B, K + 1)
    rows = ~off & ratio & ((tt > 0) | (tq > 0))
    assert rows.sum() >= 32
    seen = set()
    for b in torch.nonzero(rows).flatten().tolist():
        rej = [i for i in range(K) if not (float(u[b, i]) <= float(ap[b, i]))]
        want = rej[0] if rej else K
        assert int(acc[b]) == want, (b, u[b].tolist(), ap[b].tolist())
        seen.add(want)
    assert len(seen) >= 3                                                                 # rejections at several depths and full acceptance
    assert (rec[rows & (tt > 0)] != rec0[rows & (tt > 0)]).any()                          # (the seeded sequences do draw from another stream)
    # invariance of the seeded sequences: permuted, a smaller batch, another rng word and salt
    on = ~off
    perm = torch.randperm(B)
    a2, r2, _, _ = run_verify(H, S, lp[perm], lq[perm], spec[perm], tt[perm], tq[perm], ratio[perm], seeds[perm], pos[perm])
    assert torch.equal(a2[on[perm]], acc[perm][on[perm]]) and torch.equal(r2[on[perm]], rec[perm][on[perm]])
    sub = torch.nonzero(on).flatten()[5::3]
    a3, r3, _, _ = run_verify(H, S, lp[sub], lq[sub], spec[sub], tt[sub], tq[sub], ratio[sub], seeds[sub], pos[sub])
    assert torch.equal(a3, acc[sub]) and torch.equal(r3, rec[sub])
    a4, r4, _, _ = run_verify(H, S, lp, lq, spec, tt, tq, ratio, seeds, pos, st=424242, salt=9)
    assert torch.equal(a4[on], acc[on]) and torch.equal(r4[on], rec[on])


def test_seeded_speculative_sampling_emits_the_targets_distribution(H, S):
    """Draft tokens drawn from q with (seed, DRAFT), verified against p with the same seeds and positions (ACCEPT, TARGET): the
    first emitted token -- x_1 when accepted, else the recovery token -- is distributed as p_0 (the p, q of
    test_verify_ratio_distributions), over seeds at one position and over positions under one seed."""
    torch.manual_seed(2)
    V, K, N = 48, 3, 40000
    lp1 = (torch.randn(K + 1, V) * 1.2).to(BF)
    lq1 = (lp1[:K].float() + torch.randn(K, V) * 0.8).to(BF)
    Tt, Tq = 0.9, 1.1
    p0 = torch.softmax(lp1[0].float() / Tt, -1)
    lp, lq = lp1.unsqueeze(0).repeat(N, 1, 1).contiguous(), lq1.unsqueeze(0).repeat(N, 1, 1).contiguous()
    tt, tq = torch.full((N,), Tt), torch.full((N,), Tq)
    n = torch.arange(N, dtype=I64)
    steps = torch.arange(K + 1, dtype=I64)
    for what, seeds, pos0 in (("seeds", random_seeds(N, 2), torch.full((N,), 500, dtype=I64)),
                              ("positions", torch.full((N,), 31337, dtype=I64), n)):
        pos = (pos0.unsqueeze(1) + steps).contiguous()                  # [N][K+1]: the verify's input positions
        # the draft's K draws: row (b, i) decides x_{i+1} from q_i with the input at pos0 + i
        x = draw(S, dev(lq.view(N * K, V)), V, N * K, V, dev(tq), K, word(1), 1, dev(seeds), K, dev(pos[:, :K].reshape(-1)), S.DRAFT)
        spec = torch.cat([torch.zeros(N, 1, dtype=I64), x.view(N, K)], dim=1)
        acc, rec, _, ap = run_verify(H, S, lp, lq, spec, tt, tq, torch.ones(N, dtype=torch.bool), seeds, pos)
        first = torch.where(acc >= 1, spec[:, 1], rec)
        chi2_ok(torch.bincount(first, minlength=V), p0, f"first emitted token over {what}")
        rate = (acc >= 1).float().mean().item()
        print(f"{what}: first draft token accepted {rate:.3f}, mean accepted length {acc.float().mean().item():.3f}")
        assert 0.0 < rate < 1.0                                          # both branches ran
        chi2_ok(torch.bincount(x.view(N, K)[:, 0], minlength=V), torch.softmax(lq1[0].float() / Tq, -1), f"draft token over {what}")

"""SamplingParams(seed=S) through the whole engine on the GPU: a seeded request repeats its tokens whatever the engine sampled in
between, in autoregressive decoding, synchronous speculation (sampled chain, ratio verification) and asynchronous speculation (JIT
chains, sampled tree branches, cache hits); seeds are data, so other seeds replay the same graphs; and speculative sampling under
seeds still emits the target's distribution (two-sample chi-square against the UNSEEDED autoregressive engine, p > 1e-4).

The tiny configurations, KW, PROMPT, perturbed_pair, two_sample_ok and draw are those of tests/test_engine_temperature_gpu.py."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ssd_amd.hip import ops
    return ops


def cfgs():
    from ssd_amd.model_config import ModelConfig
    t = ModelConfig("llama", 256, 2, 4, 2, 64, 512, 128, 1e-5, 5e5, 1024, False)
    d = ModelConfig("llama", 128, 1, 2, 1, 64, 256, 128, 1e-5, 5e5, 1024, True)
    return t, d


KW = dict(max_model_len=128, max_num_batched_tokens=1024, kvcache_block_size=16, num_kvcache_blocks=256,
          num_draft_kvcache_blocks=256, weights_std=0.25)
PROMPT = [(5 * j + 1) % 128 for j in range(9)]


def perturbed_pair(noise: float):
    """Target weights and a draft of the same architecture whose weights are the target's plus noise: a correlated
    draft, so that both the accept and the reject/residual branches are exercised."""
    from ssd_amd import weights as W
    from ssd_amd.engine.llm_engine import hip_runner_factory
    t, _ = cfgs()
    wt = W.synthetic_state_dict(t, 0, KW["weights_std"])
    g = torch.Generator().manual_seed(99)
    wd = {k: (v.float() + noise * KW["weights_std"] * torch.randn(v.shape, generator=g)).to(v.dtype) if "norm" not in k else v
          for k, v in wt.items()}

    def factory(config, model_cfg, *, is_draft, topo, **kw):
        ws = wd if is_draft else wt
        return hip_runner_factory(config, model_cfg, is_draft=is_draft, topo=topo, weight_source=iter(ws.items()), **kw)
    return t, factory


def two_sample_ok(a: torch.Tensor, b: torch.Tensor, V: int, what: str):
    from scipy.stats import chi2_contingency
    ca, cb = torch.bincount(a, minlength=V).double(), torch.bincount(b, minlength=V).double()
    keep = (ca + cb) >= 10
    tab = torch.stack([torch.cat([ca[keep], ca[~keep].sum().view(1)]), torch.cat([cb[keep], cb[~keep].sum().view(1)])])
    tab = tab[:, tab.sum(0) > 0]
    stat, p, dof, _ = chi2_contingency(tab.numpy())
    print(f"{what}: chi2={stat:.1f} dof={dof} p={p:.4f}")
    assert p > 1e-4, f"{what}: two-sample chi-square p={p}"


def draw(eng, sps, rounds, per_round, n_new):
    """sps: one SamplingParams, or a function (round, slot) -> SamplingParams."""
    toks, lens = [], []
    for r in range(rounds):
        sp = [sps(r, b) for b in range(per_round)] if callable(sps) else sps
        out, m = eng.generate([PROMPT] * per_round, sp, use_tqdm=False)
        toks.extend(o["token_ids"][:n_new] for o in out)
        lens.extend(m.get("accepted_suffix_lens_with_recovery", []))
    return torch.tensor(toks), lens


N_NEW = 6


@pytest.fixture(scope="module")
def ar_unseeded(gpu):
    """1920 continuations of PROMPT from the unseeded autoregressive engine at temperature 0.7: the reference distribution of both
    speculative tests (drawn once; nothing in it depends on the batch size)."""
    from ssd_amd.engine.llm_engine import LLMEngine
    from ssd_amd.sampling_params import SamplingParams
    t, factory = perturbed_pair(0.03)
    ar = LLMEngine("t", hf_config=t, max_num_seqs=48, runner_factory=factory, **KW)
    a, _ = draw(ar, SamplingParams(temperature=0.7, max_new_tokens=N_NEW, ignore_eos=True), 40, 48, N_NEW)
    assert a[:, 1].unique().numel() >= 8, "degenerate test distribution"
    return a


def sp(seed=None, temperature=1.0, n=24, **kw):
    from ssd_amd.sampling_params import SamplingParams
    return SamplingParams(temperature=temperature, max_new_tokens=n, ignore_eos=True, seed=seed, **kw)


def toks(out):
    return [o["token_ids"] for o in out]


def test_autoregressive_seeded_requests_repeat_and_replay_the_same_graphs(gpu):
    from ssd_amd.engine.llm_engine import LLMEngine
    from ssd_amd.hip import seed_ops
    t, factory = perturbed_pair(0.03)
    eng = LLMEngine("t", hf_config=t, max_num_seqs=8, runner_factory=factory, **KW)
    runner = eng.model_runner
    batch = [sp(7), sp(None), sp(9)]
    first = toks(eng.generate([PROMPT] * 3, batch, use_tqdm=False)[0])
    assert any(k[0] == "decode_s_d" for k in runner.graphs)
    calls = seed_ops.LAUNCHES
    assert calls > 0
    between = toks(eng.generate([PROMPT] * 3, [sp(None)] * 3, use_tqdm=False)[0])     # nobody has a seed: the legacy launches alone
    assert seed_ops.LAUNCHES == calls
    assert any(k[0] == "decode_s" for k in runner.graphs)
    graphs = set(runner.graphs)
    second = toks(eng.generate([PROMPT] * 3, batch, use_tqdm=False)[0])
    assert second[0] == first[0] and second[2] == first[2]      # whatever the engine sampled in between
    assert second[1] != first[1]                                # the unseeded request moved on with the engine's stream
    assert first[0] != first[2]                                 # seeds 7 and 9: different streams
    assert len({tuple(x) for x in between}) == 3 and all(len(x) == 24 for x in first + between + second)
    assert set(runner.graphs) == graphs                         # nothing captured by the second seeded run
    # seeds are data: other seeds replay the same graphs, and the batch slot does not matter
    other = toks(eng.generate([PROMPT] * 3, [sp(9), sp(11), sp(7)], use_tqdm=False)[0])
    assert set(runner.graphs) == graphs
    assert other[0] == first[2] and other[2] == first[0] and other[1] not in (first[0], first[2])
    # no effect at temperature 0
    greedy = toks(eng.generate([PROMPT], sp(None, temperature=0), use_tqdm=False)[0])
    calls = seed_ops.LAUNCHES
    assert toks(eng.generate([PROMPT], sp(5, temperature=0), use_tqdm=False)[0]) == greedy
    assert seed_ops.LAUNCHES == calls
    mixed = toks(eng.generate([PROMPT] * 3, [sp(5, temperature=0), sp(7), sp(None)], use_tqdm=False)[0])
    assert mixed[0] == greedy[0]


def test_synchronous_speculation_repeats_under_seeds(gpu):
    from ssd_amd.engine.llm_engine import LLMEngine
    from ssd_amd.hip import seed_ops
    t, factory = perturbed_pair(0.03)
    eng = LLMEngine("t", hf_config=t, draft="d", draft_hf_config=t, speculate=True, speculate_k=3, max_num_seqs=8,
                    jit_speculate=True, runner_factory=factory, **KW)
    batch = [sp(100 + b, temperature=0.7) for b in range(6)] + [sp(None, temperature=0.7), sp(3, temperature=0)]

    def run():
        out, m = eng.generate([PROMPT] * 8, batch, use_tqdm=False)
        return toks(out), list(m["accepted_suffix_lens_with_recovery"])
    first, lens1 = run()
    calls = seed_ops.LAUNCHES
    eng.generate([PROMPT] * 5, sp(None, temperature=0.7, n=10), use_tqdm=False)       # an unseeded sampled batch in between
    assert seed_ops.LAUNCHES == calls
    second, lens2 = run()
    assert second[:6] == first[:6] and second[7] == first[7] and second[6] != first[6]
    assert len({tuple(x) for x in first[:6]}) == 6
    # the accepted lengths of a step belong to all eight sequences, one of them unseeded: equal when only seeded ones run
    seeded = batch[:6]
    a, la = (lambda r: (toks(r[0]), list(r[1]["accepted_suffix_lens_with_recovery"])))(eng.generate([PROMPT] * 6, seeded, use_tqdm=False))
    eng.generate([PROMPT] * 5, sp(None, temperature=0.7, n=10), use_tqdm=False)
    b, lb = (lambda r: (toks(r[0]), list(r[1]["accepted_suffix_lens_with_recovery"])))(eng.generate([PROMPT] * 6, seeded, use_tqdm=False))
    assert a == b and la == lb
    assert 1 < sum(la) / len(la) < 4 and min(la) < 4 and max(la) > 1          # accepted and rejected draft tokens


def test_same_model_draft_accepts_nearly_everything_under_seeds(gpu):
    from ssd_amd.engine.llm_engine import LLMEngine
    t, _ = cfgs()
    eng = LLMEngine("t", hf_config=t, draft="d", draft_hf_config=t, speculate=True, speculate_k=3, max_num_seqs=8,
                    jit_speculate=True, weights_seed=0, draft_weights_seed=0, **KW)
    out, m = eng.generate([PROMPT] * 8, [sp(b, temperature=0.9) for b in range(8)], use_tqdm=False)
    lens = m["accepted_suffix_lens_with_recovery"]
    # q and p come from differently tiled launches (M=1 decode vs M=4 verify): equal up to bf16 noise, so min(1,p/q) ~ 1
    assert sum(lens) / len(lens) > 3.8, lens
    assert len({tuple(o["token_ids"]) for o in out}) > 1          # rows draw independently


def test_seeded_synchronous_speculation_matches_unseeded_autoregressive_distribution(gpu, ar_unseeded):
    from ssd_amd.engine.llm_engine import LLMEngine
    t, factory = perturbed_pair(0.03)
    B, R, n_new = 48, 40, 5
    sd = LLMEngine("t", hf_config=t, draft="d", draft_hf_config=t, speculate=True, speculate_k=3, max_num_seqs=B,
                   jit_speculate=True, runner_factory=factory, **KW)
    s, lens = draw(sd, lambda r, b: sp(r * B + b, temperature=0.7, n=n_new), R, B, n_new)
    print("seeded sync: mean accepted (+recovery):", sum(lens) / len(lens))
    assert 1.4 < sum(lens) / len(lens) < 3.8          # some accepted, some rejected: both branches exercised
    for pos in range(1, n_new):
        two_sample_ok(ar_unseeded[:, pos], s[:, pos], t.vocab_size, f"seeded sync: marginal of generated position {pos}")


def async_engine(B):
    from ssd_amd.engine.llm_engine import LLMEngine
    t, factory = perturbed_pair(0.03)
    kw = dict(KW, num_draft_kvcache_blocks=256)
    return t, LLMEngine("t", hf_config=t, draft="d", draft_hf_config=t, speculate=True, speculate_k=3, max_num_seqs=B,
                        draft_async=True, async_fan_out=3, jit_speculate=True, inprocess_draft=True, runner_factory=factory, **kw)


def test_asynchronous_speculation_repeats_under_seeds(gpu):
    _, eng = async_engine(8)
    batch = [sp(500 + b, temperature=0.7) for b in range(8)]

    def run():
        st = dict(eng.draft_server.stats)
        out, m = eng.generate([PROMPT] * 8, batch, use_tqdm=False)
        now = eng.draft_server.stats
        return (toks(out), list(m["accepted_suffix_lens_with_recovery"]), [float(h) for h in m["cache_hits"]],
                now["hits"] - st["hits"], now["requests"] - st["requests"])
    first = run()
    eng.generate([PROMPT] * 5, sp(None, temperature=0.7, n=10), use_tqdm=False)       # an unseeded sampled batch in between
    second = run()
    assert second[0] == first[0], "tokens"
    assert second[1] == first[1], "accepted lengths"
    assert second[2] == first[2] and second[3:] == first[3:], "cache hits"
    assert 0 < first[3] < first[4]                      # both the cache path and the JIT path served requests
    assert len({tuple(x) for x in first[0]}) == 8


def test_seeded_asynchronous_speculation_matches_unseeded_autoregressive_distribution(gpu, ar_unseeded):
    B, R, n_new = 8, 120, N_NEW
    t, sd = async_engine(B)
    s, lens = draw(sd, lambda r, b: sp(10 ** 6 + r * B + b, temperature=0.7, n=n_new), R, B, n_new)
    st = sd.draft_server.stats
    print("seeded async: mean accepted (+recovery)", sum(lens) / len(lens), "cache hit rate", st["hits"] / max(1, st["requests"]))
    assert st["hits"] > 0 and st["hits"] < st["requests"]
    assert 1.3 < sum(lens) / len(lens) < 3.9
    for pos in range(1, n_new):
        two_sample_ok(ar_unseeded[:, pos], s[:, pos], t.vocab_size, f"seeded async: marginal of generated position {pos}")

"""SamplingParams(prompt_logprobs=N) through the whole engine on the GPU, with the tiny pair, the engine() helper, the oracle fixture
pattern and BOUND of tests/test_engine_logprob_gpu.py: autoregressive decoding, synchronous and asynchronous speculation.

The truth is the CPU oracle model of the same weights: log_softmax in float64 of its bf16 logits over the prompt, rows 0 .. n - 2 (row
i - 1 predicts prompt token i).  BOUND = 2 * LOGIT_ERR = 0.5 of that file was measured on this model family's prefill rows, which are
the rows scored here.  The rank is a count, so it is held to the counts the reference allows once every logit may move by
LOGIT_ERR: count(ref > ref_tok + BOUND) < rank <= count(ref >= ref_tok - BOUND); and to the kernel's own invariant exactly: a rank
within the top list means top_logprobs[rank - 1] IS the token's log-probability and the token is among top_ids[:rank].

Top lists that differ from the oracle's only in the order of entries the oracle puts within BOUND of each other are accepted for at
most 2 % of the positions of a run, as in that file.  The prompts (tests/prompt_logprob_ref.py ENGINE_PROMPTS) are of its family and
were chosen as it chose its own: those of a grid at which the decoder's own prefill logits, sorted on the host with none of the
log-probability code running, rank the oracle's top 5 alike at every prompt position (profiles/prompt_logprob_probe.py rows --grid);
tests/test_prompt_logprob_cpu.py checks on the CPU that the oracle's own decode rows against its prefill rows need no excuse on them."""
import numpy as np
import pytest
import torch

from tests.prompt_logprob_ref import ENGINE_LONG as LONG, ENGINE_PROMPTS as PROMPTS
from tests.test_engine_filter_gpu import engine
from tests.test_engine_logprob_gpu import BOUND, KEYS, MODES, check_records
from tests.test_engine_temperature_gpu import KW, cfgs, perturbed_pair

pytestmark = pytest.mark.gpu

N_NEW = 6
PKEYS = KEYS | {"prompt_logprobs"}
CHUNKED = PROMPTS[-2:]      # 21 and 13 tokens: 34 rows, of which 33 are walked in chunks of 8
assert [len(p) for p in CHUNKED] == [21, 13] and len(LONG) >= 33          # LONG: two full KV blocks of 16 and a partial one


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ssd_amd.hip import prompt_logprob_ops
    return prompt_logprob_ops


@pytest.fixture(scope="module")
def engines(gpu):
    t, factory = perturbed_pair(0.03)
    return {m: engine(m, factory, B=8) for m in MODES}


@pytest.fixture(scope="module")
def oracle():
    """prompt -> float64 [n - 1, V]: the oracle's raw log-softmax at rows 0 .. n - 2 of the prompt, teacher-forced; and, through
    .generated(prompt, tokens), the rows of generated positions as tests/test_engine_logprob_gpu.py's oracle gives them."""
    from oracle.model import Ctx, OracleModel
    from ssd_amd import weights as W
    torch.set_num_threads(min(16, torch.get_num_threads()))
    t, _ = cfgs()
    model = OracleModel(t, W.synthetic_state_dict(t, 0, KW["weights_std"]), 16, 16)
    cache = {}

    def rows(ids):
        key = tuple(ids)
        if key not in cache:
            T = len(ids)
            cu = torch.tensor([0, T], dtype=torch.int32)
            with torch.inference_mode():
                h = model.forward(torch.tensor(list(ids)), torch.arange(T), Ctx("prefill", slot_mapping=torch.arange(T, dtype=torch.int32), cu_q=cu, cu_k=cu))
                cache[key] = torch.log_softmax(model.compute_logits(h).double(), dim=-1).numpy()
        return cache[key]

    def prompt_rows(prompt):
        return rows(prompt)[:len(prompt) - 1]
    prompt_rows.generated = lambda prompt, tokens: rows(list(prompt) + list(tokens))[len(prompt) - 1:len(prompt) + len(tokens) - 1]
    return prompt_rows


def check_prompt(prompt, records, N, oracle, what):
    """Shape and truth of one request's prompt records; returns (positions, positions that needed the order excuse, worst error)."""
    assert len(records) == len(prompt) and records[0] is None, f"{what}: {len(records)} entries for {len(prompt)} prompt tokens"
    ref = oracle(prompt)
    V = ref.shape[1]
    excused, worst = 0, 0.0
    for i in range(1, len(prompt)):
        r, row, tok, w = records[i], ref[i - 1], prompt[i], f"{what} prompt token {i}"
        assert set(r) == {"token_id", "logprob", "rank", "top_ids", "top_logprobs"} and r["token_id"] == tok, w
        assert r["logprob"] <= 0.0, w
        print(f"{w}: logprob {r['logprob']:.4f} oracle {row[tok]:.4f} rank {r['rank']}")
        worst = max(worst, abs(r["logprob"] - row[tok]))
        assert abs(r["logprob"] - row[tok]) <= BOUND, f"{w}: logprob {r['logprob']} vs the oracle's {row[tok]}"
        assert len(r["top_ids"]) == len(r["top_logprobs"]) == min(N, V), w
        assert all(a >= b for a, b in zip(r["top_logprobs"], r["top_logprobs"][1:])), f"{w}: not descending"
        for j, lp in zip(r["top_ids"], r["top_logprobs"]):
            worst = max(worst, abs(lp - row[j]))
            assert abs(lp - row[j]) <= BOUND, f"{w}: top entry {j}: {lp} vs the oracle's {row[j]}"
        # the rank: a count, within the counts the reference allows when every logit may move by BOUND / 2
        lo, hi = int((row > row[tok] + BOUND).sum()), int((row >= row[tok] - BOUND).sum())
        assert isinstance(r["rank"], int) and lo < r["rank"] <= hi, f"{w}: rank {r['rank']} outside ({lo}, {hi}]"
        if r["rank"] <= len(r["top_ids"]):      # the invariant, exactly
            assert r["top_logprobs"][r["rank"] - 1] == r["logprob"] and tok in r["top_ids"][:r["rank"]], f"{w}: {r}"
        else:
            assert tok not in r["top_ids"] or r["top_logprobs"][r["top_ids"].index(tok)] == r["logprob"], w
        order = np.argsort(-row, kind="stable")[:N]
        if r["top_ids"] != order.tolist():
            assert all(abs(row[j] - row[o]) <= BOUND for j, o in zip(r["top_ids"], order)), \
                f"{w}: top ids {r['top_ids']} vs the oracle's {order.tolist()}"
            print(f"{w}: excused, top ids {r['top_ids']} vs the oracle's {order.tolist()}")
            excused += 1
    return len(prompt) - 1, excused, worst


def sp(n=None, **kw):
    from ssd_amd.sampling_params import SamplingParams
    return SamplingParams(**dict(dict(temperature=0, max_new_tokens=N_NEW, ignore_eos=True, prompt_logprobs=n), **kw))


def check_run(prompts, out, N, oracle, what):
    total = excused = 0
    worst = 0.0
    for i, (p, o) in enumerate(zip(prompts, out)):
        n, e, w = check_prompt(p, o["prompt_logprobs"], N, oracle, f"{what} prompt {i}")
        total, excused, worst = total + n, excused + e, max(worst, w)
    print(f"{what}: worst |logprob - oracle| {worst:.4f} (bound {BOUND}), top lists excused {excused} of {total}")
    assert excused <= 0.02 * total, f"{what}: {excused} of {total} positions needed the order excuse"


@pytest.fixture(scope="module")
def runs(engines):
    """Every mode without and with prompt_logprobs=5, generated once."""
    out = {}
    for m in MODES:
        plain, _ = engines[m].generate(PROMPTS, sp(), use_tqdm=False)
        asked, _ = engines[m].generate(PROMPTS, sp(5), use_tqdm=False)
        out[m] = (plain, asked)
    return out


@pytest.mark.parametrize("mode", MODES)
def test_asking_changes_no_token_and_the_records_are_the_oracles(runs, oracle, mode):
    plain, asked = runs[mode]
    assert [o["token_ids"] for o in asked] == [o["token_ids"] for o in plain]
    assert all(set(o) == KEYS for o in plain) and all(set(o) == PKEYS for o in asked)
    check_run(PROMPTS, asked, 5, oracle, mode)


def test_chunks_of_eight_rows_meet_the_same_bounds(engines, gpu, oracle):
    eng = engines["ar"]
    runner = eng.model_runner
    whole, _ = eng.generate(CHUNKED, sp(5), use_tqdm=False)
    n0, rows0 = gpu.LAUNCHES, runner.prompt_logprob_rows
    runner.prompt_logprob_rows = 8
    try:
        out, _ = eng.generate(CHUNKED, sp(5), use_tqdm=False)
    finally:
        runner.prompt_logprob_rows = rows0
    assert gpu.LAUNCHES == n0 + 5                      # 33 rows: four chunks of 8 and a ragged one; row 20, a last row, sits inside chunk 2
    assert [o["token_ids"] for o in out] == [o["token_ids"] for o in whole]
    check_run(CHUNKED, whole, 5, oracle, "one chunk")
    check_run(CHUNKED, out, 5, oracle, "chunks of 8")
    for a, b in zip(whole, out):                        # the same rows through GEMMs of other row counts: within the bound of each other
        for ra, rb in zip(a["prompt_logprobs"][1:], b["prompt_logprobs"][1:]):
            assert abs(ra["logprob"] - rb["logprob"]) <= BOUND and ra["token_id"] == rb["token_id"]


def test_the_prefix_cache_is_bypassed_for_the_asking_request_and_kept_for_the_next(gpu, oracle):
    _, factory = perturbed_pair(0.03)
    eng = engine("ar", factory, B=4)
    first, _ = eng.generate([LONG], sp(2), use_tqdm=False)
    n0 = gpu.LAUNCHES
    second, _ = eng.generate([LONG], sp(2), use_tqdm=False)
    assert gpu.LAUNCHES > n0                            # scored again: the two full blocks the first request left were not taken
    check_run([LONG], first, 2, oracle, "first")
    check_run([LONG], second, 2, oracle, "second")
    assert len(second[0]["prompt_logprobs"]) == len(LONG)
    for ra, rb in zip(first[0]["prompt_logprobs"][1:], second[0]["prompt_logprobs"][1:]):
        assert abs(ra["logprob"] - rb["logprob"]) <= BOUND
    assert second[0]["token_ids"] == first[0]["token_ids"]
    # a plain request afterwards still hits what they registered
    seqs = []
    add = eng.scheduler.add
    eng.scheduler.add = lambda s: (seqs.append(s), add(s))[1]
    cached = []
    alloc = eng.scheduler.block_manager.allocate
    eng.scheduler.block_manager.allocate = lambda s: (alloc(s), cached.append(s.num_cached_tokens))[0]
    try:
        n1 = gpu.LAUNCHES
        plain, _ = eng.generate([LONG], sp(), use_tqdm=False)
    finally:
        eng.scheduler.add, eng.scheduler.block_manager.allocate = add, alloc
    assert cached == [32] and gpu.LAUNCHES == n1 and set(plain[0]) == KEYS
    assert plain[0]["token_ids"] == first[0]["token_ids"]


@pytest.mark.parametrize("mode", MODES)
def test_a_mixed_batch(engines, runs, oracle, mode):
    plain = runs[mode][0]
    out, _ = engines[mode].generate(PROMPTS[:3], [sp(4), sp(), sp(0)], use_tqdm=False)
    assert set(out[1]) == KEYS and set(out[0]) == set(out[2]) == PKEYS
    assert [o["token_ids"] for o in out] == [o["token_ids"] for o in plain[:3]]
    check_prompt(PROMPTS[0], out[0]["prompt_logprobs"], 4, oracle, f"{mode} mixed 4")
    check_prompt(PROMPTS[2], out[2]["prompt_logprobs"], 0, oracle, f"{mode} mixed 0")
    assert all(r["top_ids"] == [] and r["top_logprobs"] == [] and r["rank"] >= 1 for r in out[2]["prompt_logprobs"][1:])


@pytest.mark.parametrize("mode", MODES)
def test_with_logprobs_and_under_a_repetition_penalty_the_records_stay_raw(engines, runs, oracle, mode):
    plain, asked = runs[mode]
    both, _ = engines[mode].generate(PROMPTS, sp(5, logprobs=5), use_tqdm=False)
    assert all(set(o) == PKEYS | {"logprobs", "cumulative_logprob"} for o in both)
    assert [o["token_ids"] for o in both] == [o["token_ids"] for o in plain]
    for p, o in zip(PROMPTS, both):
        check_prompt(p, o["prompt_logprobs"], 5, oracle, f"{mode} both")
        check_records(p, o["token_ids"], o["logprobs"], 5, oracle.generated, f"{mode} both")
        assert all("rank" not in r for r in o["logprobs"])
    pen, _ = engines[mode].generate(PROMPTS, sp(5, repetition_penalty=1.5), use_tqdm=False)
    assert [o["token_ids"] for o in pen] != [o["token_ids"] for o in plain]         # the penalty did act on the generation ...
    for p, o in zip(PROMPTS, pen):                                                   # ... and not on the prompt's records
        check_prompt(p, o["prompt_logprobs"], 5, oracle, f"{mode} penalised")


def test_a_single_token_prompt(engines, gpu):
    n0 = gpu.LAUNCHES
    out, _ = engines["ar"].generate([[17]], sp(3), use_tqdm=False)
    assert out[0]["prompt_logprobs"] == [None] and len(out[0]["token_ids"]) == N_NEW and gpu.LAUNCHES == n0
    out, _ = engines["sync"].generate([[17], PROMPTS[0]], sp(3), use_tqdm=False)
    assert out[0]["prompt_logprobs"] == [None] and len(out[1]["prompt_logprobs"]) == len(PROMPTS[0])


@pytest.mark.parametrize("mode", ["ar", "sync"])
def test_a_run_that_preempts_neither_loses_nor_doubles_a_record(gpu, oracle, mode, monkeypatch):
    """The monkeypatch of tests/test_engine_logprob_gpu.py's preemption test: a KV pool too small for the batch."""
    _, factory = perturbed_pair(0.03)
    eng = engine(mode, factory, B=3, num_kvcache_blocks=9, num_draft_kvcache_blocks=9)
    seqs, preempted, launches_at_prefill = [], [], []
    add, preempt = eng.scheduler.add, eng.scheduler.preempt
    monkeypatch.setattr(eng.scheduler, "add", lambda s: (seqs.append(s), add(s))[1])
    monkeypatch.setattr(eng.scheduler, "preempt", lambda s: (preempted.append(s.seq_id), preempt(s))[1])
    run = eng.model_runner.run

    def counted(batch, is_prefill, *a, **kw):
        if is_prefill:
            launches_at_prefill.append((gpu.LAUNCHES, any(s.needs_prompt_logprobs for s in batch)))
        return run(batch, is_prefill, *a, **kw)
    monkeypatch.setattr(eng.model_runner, "run", counted)
    prompts = [[(11 * i + 7 * j + 3) % 128 for j in range(30 + 3 * i)] for i in range(4)]
    n0 = gpu.LAUNCHES
    out, _ = eng.generate(prompts, sp(2, max_new_tokens=24), use_tqdm=False)
    assert preempted, "the pool was large enough: nothing was preempted"
    for p, o, s in zip(prompts, out, seqs):
        assert len(o["prompt_logprobs"]) == len(p) == s.num_request_prompt_tokens and o["prompt_logprobs"] is s.prompt_logprob_records
        check_prompt(p, o["prompt_logprobs"], 2, oracle, f"{mode} preempted seq {s.seq_id}")
    assert any(s.num_prompt_tokens > s.num_request_prompt_tokens for s in seqs)
    # the kernel ran in the first prefill of every request only: a re-prefill finds the records and launches nothing
    scoring = [n for n, need in launches_at_prefill if need]
    assert len(launches_at_prefill) > len(scoring) >= 1
    end = launches_at_prefill[1:] + [(gpu.LAUNCHES, False)]
    for (n, need), (n_next, _) in zip(launches_at_prefill, end):
        assert (n_next > n) == need, (launches_at_prefill, gpu.LAUNCHES)
    assert gpu.LAUNCHES - n0 == len(scoring)           # prompts of 30 .. 39 rows: one chunk per scoring prefill


def test_default_parameters_launch_nothing_and_the_prefill_replays_its_graph(gpu):
    from ssd_amd.sampling_params import SamplingParams
    _, factory = perturbed_pair(0.03)
    eng = engine("ar", factory, B=4)
    runner = eng.model_runner
    n0 = gpu.LAUNCHES
    plain = SamplingParams(temperature=0, max_new_tokens=2, ignore_eos=True)
    outs = [eng.generate([PROMPTS[1]], plain, use_tqdm=False)[0] for _ in range(3)]      # eager, captured, replayed
    assert gpu.LAUNCHES == n0 and runner.prompt_logprobs is None and all(set(o[0]) == KEYS for o in outs)
    keys = [k for k in runner.graphs if k[0] == "prefill"]
    assert len(keys) == 1
    replays = []
    g = runner.graphs[keys[0]]
    real = g.replay
    g.replay = lambda: (replays.append(1), real())[1]
    try:
        again, _ = eng.generate([PROMPTS[1]], plain, use_tqdm=False)
        asked, _ = eng.generate([PROMPTS[1]], sp(1, max_new_tokens=2), use_tqdm=False)        # the same shape, asking: eager, not the graph
        after, _ = eng.generate([PROMPTS[1]], plain, use_tqdm=False)
    finally:
        g.replay = real
    assert len(replays) == 2 and gpu.LAUNCHES == n0 + 1
    assert [k for k in runner.graphs if k[0] == "prefill"] == keys                  # asking captured nothing
    assert again[0]["token_ids"] == asked[0]["token_ids"] == after[0]["token_ids"] == outs[0][0]["token_ids"]

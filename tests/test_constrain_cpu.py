"""min_tokens / stop_token_ids / allowed_token_ids / bad_words_ids, the parts that need no GPU: SamplingParams validation, Sequence's
derived tail / min_left / bitmask against a recomputation from token_ids, stop ids through the real engine on the CPU oracle runners
(autoregressive, synchronous, asynchronous), the refusal of the kernel-needing parameters by those runners, the numpy restatement's own
hand-checked cases, and the C ABI of include/ssd_hip_constrain.h."""
import os
import random
import re
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT
from tests import constrain_ref as R

HEADER = os.path.join(ROOT, "include", "ssd_hip_constrain.h")


# ---------------------------------------------------------------------------------------------------------------------
# public interface
# ---------------------------------------------------------------------------------------------------------------------
def test_defaults_are_off():
    from ssd_amd.sampling_params import SamplingParams
    from ssd_amd.engine.sequence import Sequence
    sp = SamplingParams()
    assert (sp.stop_token_ids, sp.min_tokens, sp.allowed_token_ids, sp.bad_words_ids) == (None, 0, None, None)
    assert sp.active_constraints == []
    assert SamplingParams(stop_token_ids=[5]).active_constraints == []          # host work: no kernel needed
    assert SamplingParams(bad_words_ids=[]).active_constraints == []
    s = Sequence([1, 2, 3], sp)
    assert not s.has_constraint and s.stop_token_ids == () and s.stop_reason is None
    sp = SamplingParams(stop_token_ids=[5, 5, 6], min_tokens=3, allowed_token_ids=[9, 1, 9, 5], bad_words_ids=[[1], [2, 3], [2, 3]])
    assert sp.active_constraints == ["min_tokens", "allowed_token_ids", "bad_words_ids"]
    s = Sequence([1, 2, 3], sp)
    assert s.has_constraint and s.stop_token_ids == (5, 6) and s.allowed_token_ids == [1, 5, 9] and s.bad_words == ((1,), (2, 3))
    assert s.bad_words_flat == ([1, 2, 3], [0, 1, 3])
    assert s.stop_list(7) == [5, 6, 7] and s.stop_list(5) == [5, 6]
    assert Sequence([1], SamplingParams(ignore_eos=True, min_tokens=1, stop_token_ids=[4])).stop_list(7) == [4]
    for kw in (dict(min_tokens=1), dict(allowed_token_ids=[0]), dict(bad_words_ids=[[4]])):
        assert Sequence([1], SamplingParams(**kw)).has_constraint


@pytest.mark.parametrize("bad, name", [
    (dict(stop_token_ids=5), "stop_token_ids"), (dict(stop_token_ids=[-1]), "stop_token_ids"), (dict(stop_token_ids=[1.5]), "stop_token_ids"),
    (dict(stop_token_ids=[True]), "stop_token_ids"), (dict(stop_token_ids=list(range(65))), "stop_token_ids"),
    (dict(min_tokens=-1), "min_tokens"), (dict(min_tokens=1.0), "min_tokens"), (dict(min_tokens=True), "min_tokens"),
    (dict(min_tokens=257), "min_tokens"), (dict(min_tokens=5, max_new_tokens=4), "max_new_tokens"),
    (dict(allowed_token_ids=[]), "allowed_token_ids"), (dict(allowed_token_ids=[-3]), "allowed_token_ids"),
    (dict(allowed_token_ids={1: 2}), "allowed_token_ids"), (dict(allowed_token_ids=["1"]), "allowed_token_ids"),
    (dict(bad_words_ids=[[]]), "bad_words_ids"), (dict(bad_words_ids=[3]), "bad_words_ids"), (dict(bad_words_ids=[[-1]]), "bad_words_ids"),
    (dict(bad_words_ids=[[1, 2.0]]), "bad_words_ids"), (dict(bad_words_ids=[[i] for i in range(129)]), "bad_words_ids.*128"),
    (dict(bad_words_ids=[list(range(17))]), "bad_words_ids.*16"), (dict(bad_words_ids=[list(range(16))] * 65), "bad_words_ids.*1024"),
    (dict(allowed_token_ids=[4, 5], bad_words_ids=[[5], [4], [4, 6]]), "allowed_token_ids"),
    (dict(allowed_token_ids=[4, 5, 6], bad_words_ids=[[6]], stop_token_ids=[5, 4], min_tokens=1), "allowed_token_ids.*min_tokens"),
])
def test_every_validation_error_names_its_field(bad, name):
    from ssd_amd.sampling_params import SamplingParams
    with pytest.raises(ValueError, match=name):
        SamplingParams(**bad)


def test_the_limits_themselves_are_accepted():
    from ssd_amd.sampling_params import SamplingParams
    SamplingParams(stop_token_ids=list(range(64)), min_tokens=256, bad_words_ids=[list(range(16))] * 64)
    SamplingParams(bad_words_ids=[[i] for i in range(128)], allowed_token_ids=[128])
    SamplingParams(allowed_token_ids=[4, 5], bad_words_ids=[[5], [4, 6]], stop_token_ids=[5], min_tokens=1)      # 4 is left
    SamplingParams(allowed_token_ids=[4], stop_token_ids=[4])          # without min_tokens a stop id may be the only allowed one


# ---------------------------------------------------------------------------------------------------------------------
# Sequence bookkeeping: derived from token_ids, so nothing can go stale
# ---------------------------------------------------------------------------------------------------------------------
def test_tail_min_left_and_mask_equal_a_recomputation_from_token_ids():
    from ssd_amd.engine.sequence import Sequence
    from ssd_amd.sampling_params import SamplingParams
    rng = random.Random(11)
    for trial in range(30):
        V = rng.choice([40, 1000, 4136])
        prompt = [rng.randrange(V) for _ in range(rng.randrange(1, 30))]
        mt = rng.randrange(0, 12)
        allowed = [rng.randrange(V + 40) for _ in range(rng.randrange(1, 20))] + [V - 1, 0]
        s = Sequence(prompt, SamplingParams(min_tokens=mt, allowed_token_ids=allowed, bad_words_ids=[[1, 2]], max_new_tokens=256))
        P = len(prompt)

        def check(upto=None):
            ids = s.token_ids[:upto]
            assert s.constraint_tail(15, upto) == ids[-15:]
            assert s.num_output_tokens(upto) == max(0, len(ids) - P)
            assert s.min_left(upto) == max(0, mt - max(0, len(ids) - P))
        check()
        for step in range(25):
            op = rng.randrange(4)
            if op == 0:
                s.append_token(rng.randrange(V))
            elif op == 1:       # one speculation round: recovery + K lookahead entries, the verify's view K back, rollback, commit
                K = rng.randrange(1, 5)
                snap = s.snapshot()
                s.append_token(rng.randrange(V))
                check()
                for _ in range(K):
                    s.append_token(-1)
                check(len(s.token_ids) - K)
                s.restore(snap)
                check()
                suffix = [rng.randrange(V) for _ in range(rng.randrange(1, K + 2))]
                s.token_ids.extend(suffix)
                s.num_tokens += len(suffix)
                s.last_token = suffix[-1]
            elif op == 2:       # preemption: completions become prompt for the scheduler, not for min_tokens
                s.num_prompt_tokens = s.num_tokens
                s.num_cached_tokens = s.num_draft_cached_tokens = 0
            check()
        bits = s.allow_bits(V)
        assert bits.dtype == np.uint32 and bits.shape == ((V + 31) // 32,)
        assert (bits == R.mask_of(allowed, V)).all()
        assert s.allow_bits(V) is bits              # built once
        want = sorted({t for t in allowed if t < V})
        got = [t for t in range(32 * len(bits)) if (int(bits[t >> 5]) >> (t & 31)) & 1]
        assert got == want                          # nothing at or past V in the last partial word
        if V % 32:
            assert int(bits[-1]) >> (V % 32) == 0 and (int(bits[-1]) >> ((V - 1) % 32)) & 1


def test_stops_at_respects_min_tokens_and_ignore_eos():
    from ssd_amd.engine.sequence import Sequence
    from ssd_amd.sampling_params import SamplingParams
    s = Sequence([1, 2, 3], SamplingParams(stop_token_ids=[7], min_tokens=2))
    assert not s.stops_at(7, 3, 9) and not s.stops_at(9, 4, 9)          # output tokens 0 and 1: too early
    assert s.stops_at(7, 5, 9) and s.stops_at(9, 5, 9) and not s.stops_at(8, 5, 9)
    s = Sequence([1, 2, 3], SamplingParams(stop_token_ids=[7], ignore_eos=True))
    assert s.stops_at(7, 3, 9) and not s.stops_at(9, 3, 9)


# ---------------------------------------------------------------------------------------------------------------------
# stop ids through the engine on the CPU oracle runners
# ---------------------------------------------------------------------------------------------------------------------
K_CPU, F_CPU = 3, 2
PROMPTS = [[1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11], [3, 4, 5, 6, 7, 8, 9], [20, 30, 40]]
N_NEW = 24


@pytest.fixture(scope="module")
def cpu_engines():
    from oracle.runner import oracle_runner_factory
    from ssd_amd.engine.llm_engine import LLMEngine
    from ssd_amd.model_config import ModelConfig
    t = ModelConfig("llama", 64, 2, 4, 2, 32, 128, 256, 1e-5, 5e5, 1024, False)
    base = dict(hf_config=t, max_num_seqs=4, max_num_batched_tokens=256, kvcache_block_size=16, num_kvcache_blocks=40,
                num_draft_kvcache_blocks=40, weights_std=0.1, max_model_len=256)
    out = {}
    for mode in ("ar", "sync", "async"):
        kw = dict(base)
        if mode != "ar":
            kw.update(draft="d", draft_hf_config=t, draft_weights_seed=0, speculate=True, speculate_k=K_CPU)
        if mode == "async":
            kw.update(draft_async=True, async_fan_out=F_CPU, jit_speculate=True, inprocess_draft=True)
        out[mode] = LLMEngine("t", runner_factory=oracle_runner_factory(), **kw)
    return out


def _sp(**kw):
    from ssd_amd.sampling_params import SamplingParams
    return SamplingParams(**dict(dict(temperature=0, max_new_tokens=N_NEW, ignore_eos=True), **kw))


def _mid_suffix_stop(eng, prompt, mode):
    """(plain stream, index i, token): the token's first occurrence in the unconstrained stream is at i, strictly inside an accepted
    suffix (something follows it in the same round) when the engine speculates."""
    out, m = eng.generate([prompt], _sp(), use_tqdm=False)
    plain = out[0]["token_ids"]
    assert "stop_reason" not in out[0] and out[0]["finish_reason"] == "stop"
    ends, n = set(), 0
    for ln in m["accepted_suffix_lens_with_recovery"]:
        n += ln
        ends.add(n - 1)             # stream index of each round's last committed token
    for i in range(1, len(plain) - 1):
        if plain[i] not in plain[:i] and (mode == "ar" or i not in ends):
            return plain, i, plain[i]
    raise AssertionError(f"no usable stop token in {plain} (round ends {sorted(ends)})")


@pytest.mark.parametrize("mode", ["ar", "sync", "async"])
def test_stop_token_ids_end_each_stream_at_the_first_stop_id(cpu_engines, mode):
    eng = cpu_engines[mode]
    plain, i, tok = _mid_suffix_stop(eng, PROMPTS[0], mode)
    if mode != "ar":
        assert len(plain) > i + 1           # the accepted suffix went on behind it: the rest is what gets clipped
    out, _ = eng.generate([PROMPTS[0]], _sp(stop_token_ids=[tok]), use_tqdm=False)         # ignore_eos=True: stop ids still apply
    assert out[0]["token_ids"] == plain[:i + 1] and out[0]["stop_reason"] == tok and out[0]["finish_reason"] == "stop"
    # a batch, several ids, one request whose ids never occur, one without stop ids
    full, _ = eng.generate(PROMPTS, _sp(), use_tqdm=False)
    full = [o["token_ids"] for o in full]
    stops = [full[0][2], full[1][5], full[2][1]]
    never = next(t for t in range(256) if all(t not in f for f in full))
    params = [_sp(stop_token_ids=stops), _sp(stop_token_ids=stops), _sp(stop_token_ids=[never]), _sp()]
    out, _ = eng.generate(PROMPTS + [PROMPTS[2]], params, use_tqdm=False)
    for o, f in zip(out[:2], full[:2]):
        cut = min(f.index(t) for t in stops if t in f)
        assert o["token_ids"] == f[:cut + 1] and o["stop_reason"] == f[cut]
    assert out[2]["token_ids"] == full[2] and out[2]["stop_reason"] is None
    assert out[3]["token_ids"] == full[2] and "stop_reason" not in out[3]
    assert len(eng.scheduler.block_manager.free_block_ids) == 40           # every block went back


def test_kernel_parameters_are_refused_by_the_cpu_runners_by_name(cpu_engines):
    for eng in cpu_engines.values():
        assert not getattr(eng.model_runner, "supports_logit_constraints", False)
        for kw, name in ((dict(min_tokens=2), "min_tokens"), (dict(allowed_token_ids=[1, 2]), "allowed_token_ids"),
                         (dict(bad_words_ids=[[1, 2]]), "bad_words_ids"), (dict(allowed_token_ids=[1], bad_words_ids=[[2]]), "allowed_token_ids")):
            with pytest.raises(ValueError, match=name):
                eng.add_request([1, 2, 3], _sp(**kw))
        assert eng.is_finished()            # nothing was queued by the refused requests
    from ssd_amd.engine.model_runner import ModelRunner
    from ssd_amd.engine.eagle_runner import EagleDraftRunner
    assert ModelRunner.supports_logit_constraints and EagleDraftRunner.supports_logit_constraints


def test_add_request_checks_what_needs_the_vocabulary_and_the_eos(cpu_engines):
    """The halves SamplingParams cannot do; the runner check comes first, so it is switched on for the length of this test."""
    eng = cpu_engines["ar"]
    cls = type(eng.model_runner)
    cls.supports_logit_constraints = True
    saved, eng.config.eos = eng.config.eos, 7
    try:
        eos = eng.config.eos
        with pytest.raises(ValueError, match="allowed_token_ids.*256"):
            eng.add_request([1, 2, 3], _sp(allowed_token_ids=[5, 256]))
        with pytest.raises(ValueError, match="allowed_token_ids.*min_tokens"):
            eng.add_request([1, 2, 3], _sp(allowed_token_ids=[eos], min_tokens=1, ignore_eos=False))
        with pytest.raises(ValueError, match="min_tokens.*64"):
            eng.add_request([1, 2, 3], _sp(stop_token_ids=[t for t in range(100) if t != eos][:64], min_tokens=1, ignore_eos=False))
        assert eng.is_finished()
    finally:
        eng.config.eos = saved
        del cls.supports_logit_constraints


# ---------------------------------------------------------------------------------------------------------------------
# the reference itself, on cases small enough to check by hand
# ---------------------------------------------------------------------------------------------------------------------
def test_reference_on_hand_made_cases():
    V = 10
    assert R.mask_words(1000) == 32 and R.mask_words(4136) == 130 and R.mask_words(32) == 1
    m = R.mask_of([0, 3, 9, 10, -1], V)
    assert m.tolist() == [0b1000001001]
    assert R.banned(V, [], 0, allow=m) == {1, 2, 4, 5, 6, 7, 8}
    assert R.banned(V, [], 0, min_left=1, stops=[2, 11, -1]) == {2} and R.banned(V, [], 1, min_left=1, stops=[2]) == set()
    assert R.banned(V, [], 1, min_left=2, stops=[2]) == {2}
    assert R.banned(V, [], 0, words=[[4]]) == {4}
    assert R.banned(V, [7, 5], 0, words=[[5, 6]]) == {6} and R.banned(V, [5, 7], 0, words=[[5, 6]]) == set()
    assert R.banned(V, [5], 0, words=[[7, 5, 6]]) == set()          # the word is longer than the context
    assert R.banned(V, [7, 5], 0, words=[[7, 5, 6], [5, 6], [3, 5, 1], [5, 12]]) == {6}
    assert R.extras_seen([9, 1, 2, 3], 2, None) == [1, 2] and R.extras_seen([9, 1, 2, 3], 0, None) == []
    assert R.extras_seen([9, 1, 2, 3], 3, 7) == [1, 2, 3] and R.extras_seen([9, 1, 2, 3], 0, -2) == [] and R.extras_seen(None, 2, None) == []
    row = np.array([[0x3F80, 0x7FC1, 0x8000, 0xFF80, 0x7F80, 0x4000, 0x4040, 0x4080, 0x40A0, 0x40C0, 0x7FC5, 0x7FC5]], dtype=np.uint16)
    seqs = [dict(words=[[1], [8, 2], [8, 7, 5]], tail=[3, 8], min_left=2, stops=[9, 4])]
    out = R.constrain_rows(np.repeat(row, 3, 0), V, 3, seqs, extra=[[8, 7, 5]])
    banned_rows = [sorted(int(t) for t in np.nonzero(o != row[0])[0]) for o in out]
    # row 0: context 3 8 -> word (8, 2) bans 2; min_left bans 9 and 4; word (1) bans 1 (NaN -> -inf); entry 3 was -inf already
    # row 1: context 3 8 7 -> (8, 7, 5) bans 5 across the boundary; one extra < min_left 2;  row 2: context 3 8 7 5: nothing matches
    assert banned_rows == [[1, 2, 4, 9], [1, 4, 5, 9], [1]]
    assert (out[:, 10:] == 0x7FC5).all() and (out[0, [1, 2, 4, 9]] == 0xFF80).all() and out[2, 2] == 0x8000
    assert R.flatten_words([[1], [8, 2], [8, 7, 5]]) == ([1, 8, 2, 8, 7, 5], [0, 1, 3, 6])


# ---------------------------------------------------------------------------------------------------------------------
# C ABI
# ---------------------------------------------------------------------------------------------------------------------
def _built_lib():
    from ssd_amd.hip.lib import build_library, lib_path
    if not os.path.exists(lib_path()):
        build_library()
    return lib_path()


def constrain_header_symbols():
    return sorted(set(re.findall(r"^int\s+(ssd_\w+)\s*\(", open(HEADER).read(), flags=re.M)))


def test_constrain_header_symbols_exported_bound_and_documented():
    from ssd_amd.hip.lib import SIGNATURES, ABI_VERSION
    from ssd_amd.hip import constrain_ops as HC
    from ssd_amd import sampling_params as SP
    _built_lib()
    lib = HC.load_constrain_library()
    syms = constrain_header_symbols()
    assert syms == ["ssd_constrain_rows"] and sorted(HC.CONSTRAIN_SIGNATURES) == syms
    assert not set(syms) & set(SIGNATURES)
    assert lib.ssd_abi_version() == ABI_VERSION == 3          # additive header: the ABI version does not move
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    head = open(HEADER).read()
    for s in syms:
        assert hasattr(lib, s), f"{s} not exported"
        assert f"`{s}(" in doc, f"{s} has no line in INTEGRATION.md"
        decl = re.search(r"^int\s+" + s + r"\s*\(([^;]*)\);", head, flags=re.M | re.S).group(1)
        assert len(HC.CONSTRAIN_SIGNATURES[s]) == len(decl.split(",")), s

    def define(name):
        return int(re.search(rf"#define {name} (\d+)", head).group(1))
    pen = open(os.path.join(ROOT, "include", "ssd_hip_penalty.h")).read()          # the same bound as the penalties' extras
    assert define("SSD_CONSTRAIN_MAX_EXTRA") == HC.MAX_EXTRA == R.MAX_EXTRA == int(re.search(r"#define SSD_PENALTY_MAX_EXTRA (\d+)", pen).group(1))
    assert define("SSD_CONSTRAIN_MAX_STOP") == HC.MAX_STOP == SP.MAX_STOP_TOKEN_IDS == 64
    assert define("SSD_CONSTRAIN_MAX_WORDS") == HC.MAX_WORDS == SP.MAX_BAD_WORDS == 128
    assert define("SSD_CONSTRAIN_MAX_WORD_TOKENS") == HC.MAX_WORD_TOKENS == SP.MAX_BAD_WORD_TOKENS == 1024
    assert define("SSD_CONSTRAIN_MAX_WORD_LEN") == HC.MAX_WORD_LEN == SP.MAX_BAD_WORD_LEN == 16 and HC.TAIL_LD == 15
    assert define("SSD_CONSTRAIN_SLICE") == HC.SLICE == 4096
    common = open(os.path.join(ROOT, "ssd_amd", "csrc", "common.h")).read()
    assert '#include "ssd_hip_constrain.h"' in common
    mk = open(os.path.join(ROOT, "ssd_amd", "csrc", "Makefile")).read()
    assert "../../include/ssd_hip_constrain.h" in mk and " constrain.hip" in mk


def test_c_consumer_walks_the_constrain_validation_paths(tmp_path):
    lib = _built_lib()
    src = os.path.join(ROOT, "tests", "constrain_abi_consumer.c")
    body = open(src).read()
    for s in constrain_header_symbols():
        assert f"{s}(" in body, s
    for what in ("zero T", "T above 65535", "zero V", "zero rows_per_seq", "ld below V", "zero tail_ld", "tail_ld above", "zero extra_ld",
                 "above SSD_CONSTRAIN_MAX_EXTRA", "extra_ld below rows_per_seq", "null rows", "allow_on without allow_bits",
                 "allow_bits without allow_on", "without min_left", "without stop_len", "without bw_off", "without tail", "without tail_len",
                 "extra_n without extra"):
        assert what in body
    exe = str(tmp_path / "constrain_abi_consumer")
    libdir = os.path.dirname(lib)
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-L", libdir, "-lssdhip",
                    f"-Wl,-rpath,{libdir}", "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "0 failures" in run.stdout

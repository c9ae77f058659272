"""Repetition / presence / frequency penalties and logit bias, the parts that need no GPU: SamplingParams validation, Sequence's
incremental history table against a recount from scratch, the refusal by runners without the kernel, the numpy restatement's own
hand-checked entries, and the C ABI of include/ssd_hip_penalty.h (export, ctypes table, INTEGRATION.md, a plain-C consumer walking
the argument validation)."""
import os
import random
import re
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT
from tests import penalty_ref as R

HEADER = os.path.join(ROOT, "include", "ssd_hip_penalty.h")
NAMES = ("repetition_penalty", "presence_penalty", "frequency_penalty", "logit_bias")


# ---------------------------------------------------------------------------------------------------------------------
# public interface
# ---------------------------------------------------------------------------------------------------------------------
def test_defaults_are_off():
    from ssd_amd.sampling_params import SamplingParams
    from ssd_amd.engine.sequence import Sequence
    sp = SamplingParams()
    assert (sp.repetition_penalty, sp.presence_penalty, sp.frequency_penalty, sp.logit_bias) == (1.0, 0.0, 0.0, None)
    assert sp.active_penalties == [] and sp.active_filters == []
    assert SamplingParams(logit_bias={}).active_penalties == []
    s = Sequence([1, 2, 3], sp)
    assert not s.has_penalty and s._pen is None and not Sequence([1]).has_penalty
    with pytest.raises(AssertionError):
        s.penalty_table()
    sp = SamplingParams(repetition_penalty=1.2, presence_penalty=-0.5, frequency_penalty=0.25, logit_bias={7: -100, 9: 100.0})
    assert sp.active_penalties == list(NAMES)
    assert SamplingParams(repetition_penalty=0.5).active_penalties == ["repetition_penalty"]
    assert SamplingParams(frequency_penalty=-2).active_penalties == ["frequency_penalty"]
    s = Sequence([1, 2, 3], sp)
    assert s.has_penalty and (s.repetition_penalty, s.presence_penalty, s.frequency_penalty) == (1.2, -0.5, 0.25)
    assert s.logit_bias == {7: -100.0, 9: 100.0}
    for kw in (dict(repetition_penalty=1.1), dict(presence_penalty=0.1), dict(frequency_penalty=0.1), dict(logit_bias={0: 1.0})):
        assert Sequence([1], SamplingParams(**kw)).has_penalty


@pytest.mark.parametrize("bad", [
    dict(repetition_penalty=0.0), dict(repetition_penalty=-1.0), dict(repetition_penalty=float("nan")), dict(repetition_penalty=float("inf")),
    dict(repetition_penalty="1.2"), dict(repetition_penalty=None),
    dict(presence_penalty=float("nan")), dict(presence_penalty=float("-inf")), dict(presence_penalty="x"),
    dict(frequency_penalty=float("nan")), dict(frequency_penalty=float("inf")), dict(frequency_penalty=None),
    dict(logit_bias=[(1, 2.0)]), dict(logit_bias={-1: 1.0}), dict(logit_bias={1.5: 1.0}), dict(logit_bias={"7": 1.0}), dict(logit_bias={True: 1.0}),
    dict(logit_bias={3: float("nan")}), dict(logit_bias={3: float("inf")}), dict(logit_bias={3: 100.5}), dict(logit_bias={3: -101}),
    dict(logit_bias={3: "1"}),
])
def test_every_validation_error_names_its_field(bad):
    from ssd_amd.sampling_params import SamplingParams
    name = next(iter(bad))
    with pytest.raises(ValueError, match=name):
        SamplingParams(**bad)


def _as_ref(table):
    return {t: [e[0], e[1], e[2]] for t, e in table.items()}


def test_incremental_table_equals_a_recount_from_scratch():
    """Random prompts and appends (placeholders, lookahead that is rolled back, direct extension as the scheduler's commit does it, a
    preemption that turns completions into prompt for the scheduler), ids that also carry a bias: after every operation the table is
    the recount, and it never holds an id twice (it is a dict; its length equals the number of distinct ids)."""
    from ssd_amd.engine.sequence import Sequence
    from ssd_amd.engine.scheduler import Scheduler
    from ssd_amd.sampling_params import SamplingParams
    rng = random.Random(5)
    for trial in range(40):
        V = rng.choice([4, 16, 200])
        prompt = [rng.randrange(V) for _ in range(rng.randrange(1, 30))]
        bias = {rng.randrange(V + 5): rng.choice([-100.0, -1.5, 0.0, 3.0, 100.0]) for _ in range(rng.randrange(0, 4))}
        s = Sequence(prompt, SamplingParams(repetition_penalty=1.3, logit_bias=bias or None))
        P = len(prompt)

        def check(upto=None):
            ids = s.token_ids[:upto]
            want = R.table_of(ids[:P], ids[P:], bias)
            got = s.penalty_table(upto)
            assert _as_ref(got) == want, (trial, upto)
            assert len(got) == len({t for t in ids if t >= 0} | set(bias))
        check()
        for step in range(30):
            op = rng.randrange(6)
            if op == 0:
                s.append_token(rng.randrange(V))
            elif op == 1:                   # one speculation round: recovery + K lookahead entries, a verify that looks K back, rollback, commit
                K = rng.randrange(1, 5)
                snap = s.snapshot()
                s.append_token(rng.randrange(V))
                check()                     # the draft chain's view: everything up to the recovery token
                if rng.random() < 0.5:
                    for _ in range(K):
                        s.append_token(-1)
                else:                       # asynchronous speculation extends the list with the draft's real tokens
                    s.token_ids.extend(rng.randrange(V) for _ in range(K))
                    s.num_tokens = len(s.token_ids)
                    if rng.random() < 0.5:
                        check()             # even if somebody looked at all of it ...
                check(len(s.token_ids) - K)     # ... the verify's view ends at the recovery token
                s.restore(snap)
                check()
                suffix = [rng.randrange(V) for _ in range(rng.randrange(1, K + 2))]
                s.token_ids.extend(suffix)
                s.num_tokens += len(suffix)
                s.last_token = suffix[-1]
            elif op == 2:                   # preemption (Scheduler.preempt's effect on the sequence): the history does not move
                s.num_prompt_tokens = s.num_tokens
                s.num_cached_tokens = s.num_draft_cached_tokens = 0
            elif op == 3:
                check(rng.randrange(P, len(s.token_ids) + 1))
            check()
        assert s.num_request_prompt_tokens == P
    assert Scheduler.preempt is not None      # (the fields op 2 writes are the ones preempt writes)


def test_runners_without_the_kernel_refuse_each_parameter_by_name(golden):
    from oracle.runner import oracle_runner_factory
    from ssd_amd.engine.llm_engine import LLMEngine
    from ssd_amd.sampling_params import SamplingParams
    from tests.test_engine_cpu import mcfg, weights, COMMON
    g = golden("engine_golden")
    wt, wd = weights(g, "t."), weights(g, "d.")
    ar = LLMEngine("tiny", hf_config=mcfg(g, "t_"), runner_factory=oracle_runner_factory(wt), **COMMON)
    sd = LLMEngine("tiny", hf_config=mcfg(g, "t_"), draft="tiny-draft", draft_hf_config=mcfg(g, "d_"), speculate=True, speculate_k=3,
                   runner_factory=oracle_runner_factory(wt, wd), **COMMON)
    for eng in (ar, sd):
        assert not getattr(eng.model_runner, "supports_logit_penalties", False)
        for kw, name in ((dict(repetition_penalty=1.2), "repetition_penalty"), (dict(presence_penalty=0.5), "presence_penalty"),
                         (dict(frequency_penalty=0.5), "frequency_penalty"), (dict(logit_bias={2: 5.0}), "logit_bias"),
                         (dict(presence_penalty=0.5, logit_bias={2: 5.0}), "presence_penalty")):
            with pytest.raises(ValueError, match=name):
                eng.add_request([1, 2, 3], SamplingParams(temperature=0, **kw))
        assert eng.is_finished()                       # nothing was queued by the refused requests
    ar.add_request([1, 2, 3], SamplingParams(temperature=0, max_new_tokens=2, ignore_eos=True))
    assert not ar.is_finished()
    from ssd_amd.engine.model_runner import ModelRunner
    from ssd_amd.engine.eagle_runner import EagleDraftRunner
    assert ModelRunner.supports_logit_penalties and EagleDraftRunner.supports_logit_penalties
    assert ModelRunner.PENALTY_MAX_BIAS >= 300


# ---------------------------------------------------------------------------------------------------------------------
# the reference itself, on entries small enough to check by hand
# ---------------------------------------------------------------------------------------------------------------------
def _bits(v: float) -> int:
    return int(R.f32_to_bf16(np.float32(v))[()])


def _val(b: int) -> float:
    return float(R.bf16_to_f32(np.uint16(b))[()])


def test_reference_on_hand_made_entries():
    assert _bits(1.0) == 0x3F80 and _bits(-2.0) == 0xC000 and _val(0x4000) == 2.0
    assert _bits(1.00390625) == 0x3F80 and _bits(1.01171875) == 0x3F82          # ties go to the even mantissa
    assert R.adjust(_bits(2.0), 0.0, True, 0, 2.0, 9.0, 9.0) == _bits(1.0)          # in the prompt: r only
    assert R.adjust(_bits(-2.0), 0.0, True, 0, 2.0, 9.0, 9.0) == _bits(-4.0)
    assert R.adjust(_bits(2.0), 0.0, False, 3, 2.0, 0.5, 0.25) == _bits(1.0 - 0.75 - 0.5)
    assert R.adjust(_bits(2.0), 1.0, False, 0, 2.0, 0.5, 0.25) == _bits(3.0)          # biased and unseen: the bias alone
    assert R.adjust(_bits(2.0), -4.0, True, 1, 2.0, 0.0, 1.0) == _bits(-5.0)          # bias first: -2 is negative, so it is multiplied
    assert R.adjust(0x8000, 0.0, True, 1, 2.0, 0.0, 0.0) == 0x8000          # -0.0 is not < 0: divided, stays -0.0
    assert R.adjust(0xFF80, 100.0, True, 2, 1.5, -3.0, -3.0) == 0xFF80          # -inf stays
    assert R.adjust(0x7F80, -100.0, True, 2, 1.5, 3.0, 3.0) == 0x7F80
    for nan in (0x7FC0, 0xFFC1, 0x7F81):
        assert R.adjust(nan, 5.0, True, 2, 1.5, 3.0, 3.0) == nan
    assert R.adjust(0x7F80, 0.0, False, 2, 1.0, 0.0, 3e38) == 0x7FC0          # +inf - overflowed f * c
    row = np.array([[_bits(v) for v in (1.0, 2.0, 3.0, 4.0)] + [0x7FC5] * 2], dtype=np.uint16)
    out = R.penalize_rows(np.repeat(row, 3, 0), 4, 3, [[(1, 1, False, 0.0), (9, 1, False, 0.0), (-1, 1, False, 0.0)]], [1.0], [1.0], [0.0],
                          extra=[[0, 3, 1]])
    assert [[_val(b) for b in r[:4]] for r in out] == [[1, 1, 3, 4], [1, 1, 3, 3], [1, 1, 3, 3]]          # presence: once per distinct token
    assert (out[:, 4:] == 0x7FC5).all()
    out = R.penalize_rows(row, 4, 1, None, [1.0], [0.0], [1.0], extra=[[0, 3, 3, 2]], extra_n=2)
    assert [_val(b) for b in out[0, :4]] == [1, 2, 3, 2]          # chain form: two of the three extras, both token 3


# ---------------------------------------------------------------------------------------------------------------------
# C ABI
# ---------------------------------------------------------------------------------------------------------------------
def _built_lib():
    from ssd_amd.hip.lib import build_library, lib_path
    if not os.path.exists(lib_path()):
        build_library()
    return lib_path()


def penalty_header_symbols():
    return sorted(set(re.findall(r"^int\s+(ssd_\w+)\s*\(", open(HEADER).read(), flags=re.M)))


def test_penalty_header_symbols_exported_bound_and_documented():
    from ssd_amd.hip.lib import SIGNATURES, ABI_VERSION
    from ssd_amd.hip import penalty_ops
    _built_lib()
    lib = penalty_ops.load_penalty_library()
    syms = penalty_header_symbols()
    assert syms == ["ssd_penalize_rows"] and sorted(penalty_ops.PENALTY_SIGNATURES) == syms
    assert not set(syms) & set(SIGNATURES)             # lib.SIGNATURES stays exactly ssd_hip.h + ssd_hip_tune.h
    assert lib.ssd_abi_version() == ABI_VERSION == 3   # additive header: the ABI version does not move
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    head = open(HEADER).read()
    for s in syms:
        assert hasattr(lib, s), f"{s} not exported"
        assert f"`{s}(" in doc, f"{s} has no line in INTEGRATION.md"
        decl = re.search(r"^int\s+" + s + r"\s*\(([^;]*)\);", head, flags=re.M | re.S).group(1)
        assert len(penalty_ops.PENALTY_SIGNATURES[s]) == len(decl.split(",")), s
    assert int(re.search(r"#define SSD_PENALTY_MAX_EXTRA (\d+)", head).group(1)) == penalty_ops.MAX_EXTRA >= 16
    common = open(os.path.join(ROOT, "ssd_amd", "csrc", "common.h")).read()
    assert '#include "ssd_hip_penalty.h"' in common
    mk = open(os.path.join(ROOT, "ssd_amd", "csrc", "Makefile")).read()
    assert mk.count("../../include/ssd_hip_penalty.h") == 2 and " penalty.hip" in mk
    assert penalty_ops.pack_count(3, True) == 7 and penalty_ops.pack_count(0, False) == 0


def test_c_consumer_walks_the_penalty_validation_paths(tmp_path):
    lib = _built_lib()
    src = os.path.join(ROOT, "tests", "penalty_abi_consumer.c")
    body = open(src).read()
    for s in penalty_header_symbols():
        assert f"{s}(" in body, s
    for what in ("zero T", "zero V", "zero rows_per_seq", "ld below V", "zero tab_ld", "zero extra_ld", "above SSD_PENALTY_MAX_EXTRA",
                 "extra_ld below rows_per_seq", "null rows", "null rep", "null pres", "null freq", "without tab_len", "without tab_bias",
                 "extra_n without extra"):
        assert what in body
    exe = str(tmp_path / "penalty_abi_consumer")
    libdir = os.path.dirname(lib)
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-L", libdir, "-lssdhip",
                    f"-Wl,-rpath,{libdir}", "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "0 failures" in run.stdout

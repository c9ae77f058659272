"""Guided decoding, the parts that need no GPU: TokenAutomaton (validation by name, the limits, from_choices on hand-made cases, the
flattened tables against the numpy restatement), SamplingParams, Sequence.guide_state against a recomputation from token_ids, the refusal
of both parameters by the CPU oracle runners, what add_request checks with the vocabulary size and the EOS, the restatement's own
hand-checked cases, and the C ABI of include/ssd_hip_guide.h."""
import os
import random
import re
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT
from tests import guide_ref as R

HEADER = os.path.join(ROOT, "include", "ssd_hip_guide.h")


# ---------------------------------------------------------------------------------------------------------------------
# public interface
# ---------------------------------------------------------------------------------------------------------------------
def test_defaults_are_off_and_the_class_is_exported():
    import ssd
    import ssd_amd
    from ssd_amd.guide import TokenAutomaton
    from ssd_amd.sampling_params import SamplingParams
    from ssd_amd.engine.sequence import Sequence
    assert ssd_amd.TokenAutomaton is TokenAutomaton and ssd.TokenAutomaton is TokenAutomaton
    sp = SamplingParams()
    assert sp.guided_automaton is None and sp.guided_choice_ids is None and sp.active_guides == []
    s = Sequence([1, 2, 3], sp)
    assert s.guide is None
    a = TokenAutomaton(1, 0, {0: {4: 0}})
    assert SamplingParams(guided_automaton=a).active_guides == ["guided_automaton"]
    assert SamplingParams(guided_choice_ids=[[1, 2]]).active_guides == ["guided_choice_ids"]
    s = Sequence([1, 2, 3], SamplingParams(guided_automaton=a))
    assert s.guide is a and s.guide_state() == 0 and not s.has_constraint and not s.has_penalty


def test_delta_default_and_exception_forms():
    from ssd_amd.guide import TokenAutomaton
    a = TokenAutomaton(3, 0, {0: {5: 1, 6: -1}, 1: {7: 2, 8: -1}}, {0: 0, 2: -1})
    assert a.delta(0, 5) == 1 and a.delta(0, 6) == -1 and a.delta(0, 99) == 0          # a default with exceptions, -1 and another state
    assert a.delta(1, 7) == 2 and a.delta(1, 8) == -1 and a.delta(1, 5) == -1          # no default: the edges alone
    assert a.delta(2, 5) == -1 and a.delta(-1, 5) == -1 and a.delta(3, 5) == -1
    assert a.allowed(0, 99) and not a.allowed(0, 6) and not a.allowed(2, 0)
    assert a.any_allowed(0) and a.any_allowed(1) and not a.any_allowed(2)
    assert a.walk(0, [1, 5, 7]) == 2 and a.walk(0, [5, 5]) == -1 and a.walk(0, [5, 5, 7]) == -1
    assert a.num_states == 3 and a.num_edges == 4 and a.max_token == 8
    assert a.edge_off.tolist() == [0, 2, 4, 4] and a.dflt.tolist() == [0, -1, -1]
    assert a.edge_tok.tolist() == [5, 6, 7, 8] and a.edge_next.tolist() == [1, -1, 2, -1]
    assert all(x.dtype == np.int32 for x in (a.edge_off, a.dflt, a.edge_tok, a.edge_next))
    with pytest.raises(AttributeError):
        a.start = 1
    with pytest.raises(ValueError):
        a.edge_tok[0] = 3
    b = TokenAutomaton(2, 1, {1: {9: 0, 2: 1, 5: 0}})          # edges come out sorted by token whatever the dict's order
    assert b.edge_tok.tolist() == [2, 5, 9] and b.edge_next.tolist() == [1, 0, 0] and b.edge_off.tolist() == [0, 0, 3]


@pytest.mark.parametrize("args, name", [
    ((0, 0, {}), "num_states"), ((1.5, 0, {}), "num_states"), ((True, 0, {}), "num_states"), ((16385, 0, {0: {1: 0}}), "num_states.*16384"),
    ((2, 2, {0: {1: 0}}), "start"), ((2, -1, {0: {1: 0}}), "start"), ((2, 0, [(0, 1, 0)]), "edges"), ((2, 0, {0: [1]}), "edges"),
    ((2, 0, {2: {1: 0}}), "edges.*state 2"), ((2, 0, {0: {1: 2}}), "edges of state 0.*next state"), ((2, 0, {0: {1: -2}}), "next state"),
    ((2, 0, {0: {-1: 1}}), "edges of state 0.*token id"), ((2, 0, {0: {1.5: 1}}), "token id"), ((2, 0, {0: {2 ** 31: 1}}), "token id"),
    ((2, 0, {0: {1: 0}}, [0, 0]), "default"), ((2, 0, {0: {1: 0}}, {2: 0}), "default.*state 2"), ((2, 0, {0: {1: 0}}, {0: 2}), "default of state 0"),
    ((2, 0, {0: {1: 0}}, {0: -2}), "default of state 0"),
    ((2, 0, {1: {1: 0}}), "start state 0"), ((2, 0, {0: {1: -1}}), "start state 0"), ((2, 0, {}, {0: -1, 1: 0}), "start state 0"),
    ((1, 0, {0: {t: 0 for t in range(262145)}}), "edges.*262144"),
])
def test_every_automaton_error_names_its_argument(args, name):
    from ssd_amd.guide import TokenAutomaton
    with pytest.raises(ValueError, match=name):
        TokenAutomaton(*args)


def test_the_limits_themselves_are_accepted():
    from ssd_amd.guide import TokenAutomaton, MAX_STATES, MAX_EDGES
    from ssd_amd.sampling_params import SamplingParams
    assert (MAX_STATES, MAX_EDGES) == (16384, 262144)
    a = TokenAutomaton(MAX_STATES, MAX_STATES - 1, {MAX_STATES - 1: {t: t % MAX_STATES for t in range(MAX_EDGES)}}, {0: MAX_STATES - 1})
    assert a.num_edges == MAX_EDGES and a.edge_off[-1] == MAX_EDGES and a.delta(MAX_STATES - 1, MAX_EDGES - 1) == (MAX_EDGES - 1) % MAX_STATES
    SamplingParams(guided_automaton=a)
    TokenAutomaton(1, 0, {}, {0: 0})                                    # a default alone allows everything
    TokenAutomaton(1, 0, {0: {2 ** 31 - 1: 0}})
    # 16382 one-token choices + the start + the state behind the EOS = 16384 states
    SamplingParams(guided_choice_ids=[[t] for t in range(MAX_STATES - 2)])
    with pytest.raises(ValueError, match="guided_choice_ids.*16384"):
        SamplingParams(guided_choice_ids=[[t] for t in range(MAX_STATES - 1)])


@pytest.mark.parametrize("bad, name", [
    (dict(guided_automaton="x"), "guided_automaton"), (dict(guided_automaton={0: {1: 0}}), "guided_automaton"),
    (dict(guided_choice_ids=[]), "guided_choice_ids"), (dict(guided_choice_ids=[[]]), "guided_choice_ids"),
    (dict(guided_choice_ids=[3]), "guided_choice_ids"), (dict(guided_choice_ids=[[-1]]), "guided_choice_ids"),
    (dict(guided_choice_ids=[[1, 2.0]]), "guided_choice_ids"), (dict(guided_choice_ids=[[True]]), "guided_choice_ids"),
    (dict(guided_choice_ids="ab"), "guided_choice_ids"),
    (dict(guided_choice_ids=[[1, 2]], ignore_eos=True), "guided_choice_ids.*ignore_eos"),
])
def test_every_sampling_params_error_names_its_field(bad, name):
    from ssd_amd.sampling_params import SamplingParams
    with pytest.raises(ValueError, match=name):
        SamplingParams(**bad)


def test_both_fields_at_once_are_refused():
    from ssd_amd.guide import TokenAutomaton
    from ssd_amd.sampling_params import SamplingParams
    with pytest.raises(ValueError, match="guided_automaton and guided_choice_ids"):
        SamplingParams(guided_automaton=TokenAutomaton(1, 0, {0: {4: 0}}), guided_choice_ids=[[1]])


# ---------------------------------------------------------------------------------------------------------------------
# from_choices
# ---------------------------------------------------------------------------------------------------------------------
def test_from_choices_on_hand_made_cases():
    from ssd_amd.guide import TokenAutomaton
    EOS = 9
    # a shared prefix: 1 2 3 and 1 2 4 and 5 6
    a = TokenAutomaton.from_choices([[1, 2, 3], [1, 2, 4], [5, 6]], EOS)
    assert a.num_states == 8 and a.start == 0 and (a.dflt == -1).all()          # 0, (1), (1 2), (1 2 3), (1 2 4), (5), (5 6), final
    s12 = a.walk(0, [1, 2])
    assert sorted(t for t in range(12) if a.allowed(0, t)) == [1, 5] and sorted(t for t in range(12) if a.allowed(s12, t)) == [3, 4]
    for c in ([1, 2, 3], [1, 2, 4], [5, 6]):
        end = a.walk(0, c)
        assert [t for t in range(12) if a.allowed(end, t)] == [EOS]
        final = a.delta(end, EOS)
        assert final == a.num_states - 1 and not a.any_allowed(final)
    assert a.walk(0, [1, 2, 5]) == -1 and a.walk(0, [1, 2, 3, 3]) == -1 and a.walk(0, [EOS]) == -1
    assert a.num_edges == 6 + 3          # the trie's edges and one EOS edge per choice
    # one choice a prefix of another: the EOS and the continuation are both allowed there
    a = TokenAutomaton.from_choices([[1, 2], [1, 2, 3]], EOS)
    s12 = a.walk(0, [1, 2])
    assert sorted(t for t in range(12) if a.allowed(s12, t)) == [3, EOS]
    assert a.delta(s12, EOS) == a.delta(a.walk(0, [1, 2, 3]), EOS) == a.num_states - 1 and a.num_states == 5
    # a single one-token choice; a repeated choice changes nothing
    a = TokenAutomaton.from_choices([[7]], EOS)
    assert a.num_states == 3 and a.edge_tok.tolist() == [7, EOS] and a.edge_next.tolist() == [1, 2] and a.edge_off.tolist() == [0, 1, 2, 2]
    b = TokenAutomaton.from_choices([[7], [7]], EOS)
    assert b.edge_tok.tolist() == a.edge_tok.tolist() and b.num_states == 3
    for bad, name in (([[1, EOS, 2]], "EOS"), ([[EOS]], "EOS"), ([], "choices"), ([[]], "choices"), ([[1], 2], "choices")):
        with pytest.raises(ValueError, match=name):
            TokenAutomaton.from_choices(bad, EOS)
    with pytest.raises(ValueError, match="eos"):
        TokenAutomaton.from_choices([[1]], -1)


def _random_automaton(rng, V):
    from ssd_amd.guide import TokenAutomaton
    n = rng.randrange(1, 9)
    edges, default = {}, {}
    for s in range(n):
        toks = rng.sample(range(V), rng.randrange(0, min(V, 12)))
        edges[s] = {t: rng.randrange(-1, n) for t in toks}
        if rng.random() < 0.4:
            default[s] = rng.randrange(-1, n)
    edges[0][rng.randrange(V)] = rng.randrange(n)           # something is allowed at the start
    return TokenAutomaton(n, 0, edges, default)


def test_flattened_tables_round_trip_through_the_reference_delta():
    rng = random.Random(5)
    for trial in range(40):
        V = rng.choice([6, 40, 300])
        a = _random_automaton(rng, V)
        tab = R.tables_of(a)
        assert (np.diff(a.edge_off) >= 0).all()
        for s in range(a.num_states):
            o0, o1 = a.edge_off[s], a.edge_off[s + 1]
            assert (np.diff(a.edge_tok[o0:o1]) > 0).all()          # sorted, strictly increasing
            want = [a.delta(s, t) for t in range(V)]
            assert [R.delta(tab, s, t) for t in range(V)] == want
            assert (R.allowed_set(tab, s, V) == (np.array(want) != -1)).all()
        assert R.delta(tab, -1, 0) == -1 and R.delta(tab, a.num_states, 0) == -1


# ---------------------------------------------------------------------------------------------------------------------
# Sequence bookkeeping: derived from token_ids, so nothing can go stale
# ---------------------------------------------------------------------------------------------------------------------
def test_guide_state_equals_a_recomputation_from_token_ids():
    from ssd_amd.engine.sequence import Sequence
    from ssd_amd.sampling_params import SamplingParams
    rng = random.Random(13)
    for trial in range(40):
        V = rng.choice([4, 6, 40])
        a = _random_automaton(rng, V)
        prompt = [rng.randrange(V) for _ in range(rng.randrange(1, 20))]
        s = Sequence(prompt, SamplingParams(guided_automaton=a))
        P = len(prompt)

        def check(upto=None):
            ids = s.token_ids[:upto]
            assert all(t >= 0 for t in ids)
            assert s.guide_state(upto) == a.walk(a.start, ids[P:]), (ids, P)
        check()
        check(rng.randrange(0, P + 1))          # inside the prompt: the start state
        for step in range(25):
            op = rng.randrange(4)
            if op == 0:
                s.append_token(rng.randrange(V))
            elif op == 1:       # one speculation round: recovery + K placeholders, the verify's view K back, rollback, another suffix
                K = rng.randrange(1, 5)
                snap = s.snapshot()
                s.append_token(rng.randrange(V))
                check()
                for _ in range(K):
                    s.append_token(-1)
                check(len(s.token_ids) - K)
                s.restore(snap)
                check()
                suffix = [rng.randrange(V) for _ in range(rng.randrange(1, K + 2))]          # not the tokens the round looked at
                s.token_ids.extend(suffix)
                s.num_tokens += len(suffix)
                s.last_token = suffix[-1]
            elif op == 2:       # preemption: completions become prompt for the scheduler, not for the guide
                s.num_prompt_tokens = s.num_tokens
                s.num_cached_tokens = s.num_draft_cached_tokens = 0
            check()
            check(rng.randrange(P, len(s.token_ids) + 1))
        assert s.num_request_prompt_tokens == P


def test_a_compiled_guide_wins_over_the_params_and_a_default_sequence_keeps_none():
    from ssd_amd.guide import TokenAutomaton
    from ssd_amd.engine.sequence import Sequence
    from ssd_amd.sampling_params import SamplingParams
    a = TokenAutomaton.from_choices([[3, 4]], 9)
    s = Sequence([1, 2], SamplingParams(guided_choice_ids=[[3, 4]]), guide=a)
    assert s.guide is a
    for t in (3, 4, 9):
        s.append_token(t)
    assert s.guide_state() == a.num_states - 1 and s.guide_state(3) == 1
    snap = Sequence([1], SamplingParams())
    snap.restore(snap.snapshot())          # nothing to cut back
    assert snap.guide is None


# ---------------------------------------------------------------------------------------------------------------------
# the engine on the CPU oracle runners: both parameters are refused by name; add_request's own checks
# ---------------------------------------------------------------------------------------------------------------------
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
            kw.update(draft="d", draft_hf_config=t, draft_weights_seed=0, speculate=True, speculate_k=3)
        if mode == "async":
            kw.update(draft_async=True, async_fan_out=2, jit_speculate=True, inprocess_draft=True)
        out[mode] = LLMEngine("t", runner_factory=oracle_runner_factory(), **kw)
    return out


def _sp(**kw):
    from ssd_amd.sampling_params import SamplingParams
    return SamplingParams(**dict(dict(temperature=0, max_new_tokens=8), **kw))


def test_both_parameters_are_refused_by_the_cpu_runners_by_name(cpu_engines):
    from ssd_amd.guide import TokenAutomaton
    a = TokenAutomaton(1, 0, {0: {4: 0}})
    for eng in cpu_engines.values():
        assert not getattr(eng.model_runner, "supports_guided_decoding", False)
        for kw, name in ((dict(guided_automaton=a), "guided_automaton"), (dict(guided_choice_ids=[[1, 2]]), "guided_choice_ids")):
            with pytest.raises(ValueError, match=name):
                eng.add_request([1, 2, 3], _sp(**kw))
        assert eng.is_finished()            # nothing was queued by the refused requests
        out, _ = eng.generate([[1, 2, 3]], _sp(), use_tqdm=False)          # ... and an unguided request runs as ever
        assert len(out[0]["token_ids"]) >= 1
    from ssd_amd.engine.model_runner import ModelRunner
    from ssd_amd.engine.eagle_runner import EagleDraftRunner
    assert ModelRunner.supports_guided_decoding and EagleDraftRunner.supports_guided_decoding


def test_add_request_checks_what_needs_the_vocabulary_and_the_eos(cpu_engines):
    """The halves SamplingParams cannot do; the runner check comes first, so it is switched on for the length of this test."""
    from ssd_amd.guide import TokenAutomaton
    eng = cpu_engines["ar"]
    cls = type(eng.model_runner)
    cls.supports_guided_decoding = True
    saved, eng.config.eos = eng.config.eos, 7
    try:
        with pytest.raises(ValueError, match="guided_choice_ids.*256"):
            eng.add_request([1, 2, 3], _sp(guided_choice_ids=[[5, 256]]))
        with pytest.raises(ValueError, match="guided_automaton.*256"):
            eng.add_request([1, 2, 3], _sp(guided_automaton=TokenAutomaton(1, 0, {0: {4: 0, 256: 0}})))
        with pytest.raises(ValueError, match="guided_choice_ids.*EOS 7"):
            eng.add_request([1, 2, 3], _sp(guided_choice_ids=[[5, 7, 6]]))
        sp = _sp(guided_choice_ids=[[5, 6]])
        sp.ignore_eos = True            # a dataclass can be changed behind its own checks
        with pytest.raises(ValueError, match="guided_choice_ids.*ignore_eos"):
            eng.add_request([1, 2, 3], sp)
        sp = _sp(guided_choice_ids=[[5, 6]])
        sp.guided_automaton = TokenAutomaton(1, 0, {0: {4: 0}})
        with pytest.raises(ValueError, match="guided_automaton and guided_choice_ids"):
            eng.add_request([1, 2, 3], sp)
        eng.config.eos = -1             # an engine without a tokenizer has no EOS: a choice could not end
        with pytest.raises(ValueError, match="guided_choice_ids.*EOS"):
            eng.add_request([1, 2, 3], _sp(guided_choice_ids=[[5, 6]]))
        eng.config.eos = 7
        assert eng.is_finished()
        # what is accepted reaches the scheduler with the automaton compiled against the engine's EOS
        eng.add_request([1, 2, 3], _sp(guided_choice_ids=[[5, 255], [5]]))
        seq = eng.scheduler.waiting[-1]
        assert seq.guide is not None and seq.guide.walk(0, [5, 255, 7]) == seq.guide.num_states - 1 and seq.guide.allowed(1, 7)
        eng.scheduler.waiting.clear()
        assert eng.is_finished()
    finally:
        eng.config.eos = saved
        del cls.supports_guided_decoding


# ---------------------------------------------------------------------------------------------------------------------
# the reference itself, on cases small enough to check by hand
# ---------------------------------------------------------------------------------------------------------------------
def test_reference_on_hand_made_cases():
    V = 10
    # state 0: default 0, token 3 banned, token 4 -> 1;  state 1: edges 5 -> 2, 6 -> 3 (3 == n: reads as -1), 12 -> 0 (past V);
    # state 2: nothing
    a = R.tables_from(3, {0: [(4, 1), (3, -1)], 1: [(5, 2), (6, 3), (12, 0)]}, {0: 0})
    assert a["tok"].tolist() == [3, 4, 5, 6, 12] and a["off"].tolist() == [0, 2, 5, 5]
    assert R.delta(a, 0, 3) == -1 and R.delta(a, 0, 4) == 1 and R.delta(a, 0, 9) == 0 and R.delta(a, 1, 6) == -1 and R.delta(a, 1, 5) == 2
    assert R.delta(a, 2, 5) == -1 and R.delta(a, -1, 4) == -1 and R.delta(a, 3, 4) == -1
    assert R.allowed_set(a, 0, V).tolist() == [True, True, True, False] + [True] * 6
    assert np.nonzero(R.allowed_set(a, 1, V))[0].tolist() == [5] and not R.allowed_set(a, 2, V).any()
    assert R.extras_seen([9, 1, 2, 3], 2, None) == [1, 2] and R.extras_seen([9, 1, 2, 3], 3, 7) == [1, 2, 3] and R.extras_seen(None, 2, None) == []
    # prefix form: row j sees j extras; the walk dies at the banned 3 and stays dead
    got = R.walk(4, 4, [a], [1], [0], extra=[[8, 4, 5, 1]])
    assert got.tolist() == [0, 1, 2, -1]
    assert R.walk(4, 4, [a], [1], [0], extra=[[8, 7, 3, 4]]).tolist() == [0, 0, -1, -1]
    assert R.walk(2, 2, [a], [1], [0], extra=[[8, -1]]).tolist() == [0, -1]          # a negative extra
    # chain form: every row sees extra_n of them, clamped; guide_on 0 and a start outside the automaton give -1
    assert R.walk(2, 1, [a, a], [1, 1], [0, 1], extra=[[8, 4, 5], [8, 5, 5]], extra_n=1).tolist() == [1, 2]
    assert R.walk(2, 1, [a, a], [1, 1], [0, 1], extra=[[8, 4, 5], [8, 5, 5]], extra_n=9).tolist() == [2, -1]
    assert R.walk(3, 1, [a, a, a], [0, 1, 1], [0, 3, -1]).tolist() == [-1, -1, -1]
    row = np.array([[0x3F80, 0x7FC1, 0x8000, 0xFF80, 0x7F80, 0x4000, 0x4040, 0x4080, 0x40A0, 0x40C0, 0x7FC5, 0x7FC5]], dtype=np.uint16)
    out = R.guide_rows(np.repeat(row, 4, 0), V, 4, [a], [0, 1, 2, -1])
    changed = [sorted(int(t) for t in np.nonzero(o != row[0])[0]) for o in out]
    # state 0 bans 3 (already -inf: no change); state 1 keeps 5 alone; state 2 bans all of [0, V); -1 touches nothing
    assert changed == [[], [0, 1, 2, 4, 6, 7, 8, 9], [0, 1, 2, 4, 5, 6, 7, 8, 9], []]
    assert (out[:, 10:] == 0x7FC5).all() and (out[2, :V] == 0xFF80).all() and out[1, 5] == 0x4000
    # offsets that run backwards or leave the table: the state has no edges
    b = dict(a, off=np.array([2, 0, 9, 9]))
    assert R.edge_range(b, 0) == (0, 0) and R.edge_range(b, 1) == (0, 0) and R.delta(b, 0, 4) == 0 and R.delta(b, 1, 5) == -1


# ---------------------------------------------------------------------------------------------------------------------
# C ABI
# ---------------------------------------------------------------------------------------------------------------------
def _built_lib():
    from ssd_amd.hip.lib import build_library, lib_path
    if not os.path.exists(lib_path()):
        build_library()
    return lib_path()


def guide_header_symbols():
    return sorted(set(re.findall(r"^int\s+(ssd_\w+)\s*\(", open(HEADER).read(), flags=re.M)))


def test_guide_header_symbols_exported_bound_and_documented():
    from ssd_amd.hip.lib import SIGNATURES, ABI_VERSION
    from ssd_amd.hip import guide_ops as HG
    from ssd_amd import guide as G
    _built_lib()
    lib = HG.load_guide_library()
    syms = guide_header_symbols()
    assert syms == ["ssd_guide_rows", "ssd_guide_walk"] and sorted(HG.GUIDE_SIGNATURES) == syms
    assert not set(syms) & set(SIGNATURES)
    assert lib.ssd_abi_version() == ABI_VERSION == 3          # additive header: the ABI version does not move
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    head = open(HEADER).read()
    for s in syms:
        assert hasattr(lib, s), f"{s} not exported"
        assert f"`{s}(" in doc, f"{s} has no line in INTEGRATION.md"
        decl = re.search(r"^int\s+" + s + r"\s*\(([^;]*)\);", head, flags=re.M | re.S).group(1)
        assert len(HG.GUIDE_SIGNATURES[s]) == len(decl.split(",")), s

    def define(name, text=head):
        return int(re.search(rf"#define {name} (\d+)", text).group(1))
    con = open(os.path.join(ROOT, "include", "ssd_hip_constrain.h")).read()          # the same bounds as the constraints' extras and slices
    assert define("SSD_GUIDE_MAX_EXTRA") == HG.MAX_EXTRA == R.MAX_EXTRA == define("SSD_CONSTRAIN_MAX_EXTRA", con)
    assert define("SSD_GUIDE_SLICE") == HG.SLICE == R.SLICE == define("SSD_CONSTRAIN_SLICE", con) == 4096
    assert define("SSD_GUIDE_MAX_STATES") == HG.MAX_STATES == G.MAX_STATES == R.MAX_STATES == 16384
    assert define("SSD_GUIDE_MAX_EDGES") == HG.MAX_EDGES == G.MAX_EDGES == R.MAX_EDGES == 262144
    assert HG.MAX_EDGES == 64 ** 3          # what two narrowing rounds and a compare per lane search: also the largest edges_ld
    common = open(os.path.join(ROOT, "ssd_amd", "csrc", "common.h")).read()
    assert '#include "ssd_hip_guide.h"' in common
    mk = open(os.path.join(ROOT, "ssd_amd", "csrc", "Makefile")).read()
    assert "../../include/ssd_hip_guide.h" in mk and " guide.hip" in mk


def test_c_consumer_walks_the_guide_validation_paths(tmp_path):
    lib = _built_lib()
    src = os.path.join(ROOT, "tests", "guide_abi_consumer.c")
    body = open(src).read()
    for s in guide_header_symbols():
        assert f"{s}(" in body, s
    for what in ("zero T", "T above 65535", "zero V", "zero rows_per_seq", "ld below V", "zero states_ld", "zero edges_ld",
                 "above SSD_GUIDE_MAX_EDGES", "zero extra_ld", "above SSD_GUIDE_MAX_EXTRA", "extra_ld below rows_per_seq", "null rows",
                 "null state_rows", "null guide_on", "null state0", "without n_states", "without edge_off", "without dflt",
                 "without edge_tok", "without edge_next", "extra_n without extra"):
        assert what in body
    exe = str(tmp_path / "guide_abi_consumer")
    libdir = os.path.dirname(lib)
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-L", libdir, "-lssdhip",
                    f"-Wl,-rpath,{libdir}", "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "0 failures" in run.stdout

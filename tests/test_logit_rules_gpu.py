"""Penalties, Constraints and Guides (ssd_amd/engine/logit_rules.py) alone on the GPU, without a model: stage -> pinned -> device ->
kernel against tests/penalty_ref.py, constrain_ref.py and guide_ref.py fed with values worked out from the SamplingParams by hand.
V = 4104 is one full 4096-entry slice plus one chunk, so ids sit on each side of the slice edge."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from ssd_amd.engine.sequence import Sequence
from ssd_amd.guide import TokenAutomaton
from ssd_amd.sampling_params import SamplingParams
from tests import constrain_ref as CR
from tests import guide_ref as GR
from tests import penalty_ref as PR

pytestmark = pytest.mark.gpu

V, K, EOS, CAP = 4104, 2, 5, 8
B, RPS = 3, K + 1
PROMPT = [7, 8, 4096, 7, 40]
PLAIN = SamplingParams()


@pytest.fixture(scope="module")
def sizes():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ssd_amd.engine.logit_rules import RuleSizes
    return RuleSizes(seq_cap=CAP, vocab=V, K=K, max_model_len=64, rows=16, eos=EOS, device=torch.device("cuda"))


@pytest.fixture(scope="module")
def rows():
    """(the raw rows as bf16 bits, the round's inputs) shared by the three tests; never written."""
    rng = np.random.default_rng(11)
    bits = PR.f32_to_bf16(rng.normal(0, 3, size=(B * RPS, V)).astype(np.float32))
    extra = rng.integers(4090, V, size=(B, K + 1))
    bits.setflags(write=False)
    return bits, extra


def seq(sp, out):
    """`out` generated behind PROMPT, then the K entries of a round's lookahead."""
    s = Sequence(list(PROMPT), sp)
    for t in list(out) + [-1] * K:
        s.append_token(t)
    return s


def run(rule, seqs, stage_set, rows, base=0):
    bits, extra = rows
    lg = torch.from_numpy(bits.view(np.int16).copy()).cuda().view(torch.bfloat16)
    rule.stage(seqs, K, stage_set, base)
    rule.apply(lg, B * RPS, RPS, dict(extra=torch.from_numpy(extra).cuda(), extra_ld=K + 1), base)
    torch.cuda.synchronize()
    return lg.view(torch.int16).cpu().numpy().view(np.uint16)


def history(s):
    return s.token_ids[len(PROMPT):len(s.token_ids) - K]


def untouched(got, rows, b):
    return np.array_equal(got[b * RPS:(b + 1) * RPS], rows[0][b * RPS:(b + 1) * RPS])


# ---- penalties ---------------------------------------------------------------------------------------------------------------------
def want_penalties(seqs, rows):
    tabs, par = [], []
    for s in seqs:
        if not s.has_penalty:
            tabs.append([])
            par.append((1.0, 0.0, 0.0))
            continue
        tab = PR.table_of(PROMPT, history(s), s.logit_bias)
        tabs.append([(t, c, ip, b) for t, (c, ip, b) in tab.items()])
        par.append((s.repetition_penalty, s.presence_penalty, s.frequency_penalty))
    return PR.penalize_rows(rows[0], V, RPS, tabs, *np.array(par, np.float32).T, extra=rows[1])


def test_penalties_staged_and_applied_alone(sizes, rows):
    from ssd_amd.engine.logit_rules import Penalties
    rule = Penalties(sizes)
    a = SamplingParams(repetition_penalty=1.3, presence_penalty=0.25, frequency_penalty=0.5, logit_bias={4095: 2.5, 4096: -1.0, 4103: 7.0})
    c = SamplingParams(frequency_penalty=-0.75, logit_bias={0: 1.0})
    first = [seq(a, [40, 4095, 4095, 33]), seq(c, [4096, 4100]), seq(a, [9])]
    got = run(rule, first, 0, rows)
    assert np.array_equal(got, want_penalties(first, rows)) and not any(untouched(got, rows, b) for b in range(B))
    second = [seq(c, [4097, 4097, 4098]), seq(a, [4103]), seq(c, [])]
    assert np.array_equal(run(rule, second, 1, rows), want_penalties(second, rows))
    third = [first[0], seq(PLAIN, [11, 12]), first[2]]
    got = run(rule, third, 0, rows)
    assert np.array_equal(got, want_penalties(third, rows)) and untouched(got, rows, 1) and not untouched(got, rows, 0)


# ---- constraints -------------------------------------------------------------------------------------------------------------------
def want_constraints(seqs, rows):
    ref = []
    for s in seqs:
        if not s.has_constraint:
            ref.append({})
            continue
        ref.append(dict(allow=CR.mask_of(s.allowed_token_ids, V) if s.allowed_token_ids is not None else None,
                        min_left=max(0, s.min_tokens - len(history(s))), stops=list(s.stop_token_ids) + [EOS],
                        words=[list(w) for w in s.bad_words], tail=s.token_ids[:len(s.token_ids) - K]))
    return CR.constrain_rows(rows[0], V, RPS, ref, extra=rows[1])


def test_constraints_staged_and_applied_alone(sizes, rows):
    from ssd_amd.engine.logit_rules import Constraints
    rule = Constraints(sizes)
    a = SamplingParams(min_tokens=4, stop_token_ids=[4095, 4096], allowed_token_ids=[t for t in range(3, V) if t % 5], bad_words_ids=[[4103], [33, 4097]])
    c = SamplingParams(bad_words_ids=[[4095], [4096], [4091, 4092, 4099]])
    m = SamplingParams(min_tokens=2, stop_token_ids=[4101])
    first = [seq(a, [40, 4094, 33]), seq(c, [4096, 4100]), seq(m, [9])]
    got = run(rule, first, 0, rows)
    assert np.array_equal(got, want_constraints(first, rows)) and not any(untouched(got, rows, b) for b in range(B))
    assert got[0, 4095] == CR.NINF and got[0, 4096] == CR.NINF and got[0, 4097] == CR.NINF and got[3, 4095] == CR.NINF
    assert rule.owner[:B] == [first[0].seq_id, None, None]
    second = [seq(m, []), seq(a, [4102]), seq(c, [4091, 4092])]
    assert np.array_equal(run(rule, second, 1, rows), want_constraints(second, rows))
    third = [first[0], seq(PLAIN, [11, 12]), first[2]]
    got = run(rule, third, 0, rows)
    assert np.array_equal(got, want_constraints(third, rows)) and untouched(got, rows, 1) and not untouched(got, rows, 0)


# ---- guides ------------------------------------------------------------------------------------------------------------------------
def want_guides(seqs, rows):
    autos, on, s0 = [], [], []
    for s in seqs:
        a = s.guide
        st = a.start if a is not None else 0
        for t in (history(s) if a is not None else []):
            st = a.delta(st, t)
        autos.append(GR.tables_of(a) if a is not None else None)
        on.append(int(a is not None))
        s0.append(st)
    return GR.guide_rows(rows[0], V, RPS, autos, GR.walk(B * RPS, RPS, autos, on, s0, extra=rows[1]))


def test_guides_staged_and_applied_alone(sizes, rows):
    from ssd_amd.engine.logit_rules import Guides
    rule = Guides(sizes)
    residues = SamplingParams(guided_automaton=TokenAutomaton(3, 0, {s: {t: t % 3 for t in range(V) if t % 3 != s} for s in range(3)}))
    # everything but the two ids at the slice edge, from a default; 4100 leads to a state that allows 4095 and 4096 alone
    edge = SamplingParams(guided_automaton=TokenAutomaton(2, 0, {0: {4095: -1, 4096: -1, 4100: 1}, 1: {4095: 0, 4096: 0}}, default={0: 0}))
    first = [seq(residues, [1, 2, 4096]), seq(edge, [4100]), seq(edge, [9, 4100, 4095])]
    got = run(rule, first, 0, rows)
    assert np.array_equal(got, want_guides(first, rows)) and not any(untouched(got, rows, b) for b in range(B))
    assert rule.owner[:B] == [s.seq_id for s in first]
    second = [seq(edge, []), seq(residues, [4097]), seq(residues, [1, 1])]         # the last one left its guide: state -1
    got = run(rule, second, 1, rows)
    assert np.array_equal(got, want_guides(second, rows)) and untouched(got, rows, 2)
    third = [first[0], seq(PLAIN, [11, 12]), first[2]]
    got = run(rule, third, 0, rows)
    assert np.array_equal(got, want_guides(third, rows)) and untouched(got, rows, 1) and not untouched(got, rows, 0)
    assert rule.owner[:B] == [first[0].seq_id, second[1].seq_id, first[2].seq_id]
    # the prefill's slots: the last B, which leaves the owners of the first ones alone
    arrivals = [seq(edge, []), seq(residues, []), seq(edge, [])]
    got = run(rule, arrivals, 0, rows, base=CAP - B)
    assert np.array_equal(got, want_guides(arrivals, rows))
    assert rule.owner[:B] == [first[0].seq_id, second[1].seq_id, first[2].seq_id] and rule.owner[CAP - B:] == [s.seq_id for s in arrivals]

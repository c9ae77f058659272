"""The host half of ssd_amd/engine/logit_rules.py without a GPU: the numpy packers against the references of the three kernels
(tests/penalty_ref.py, constrain_ref.py, guide_ref.py), the stale-row clearing, the limits, the slot owner, the Sampling names and
lib.bind.  The packers fill plain numpy arrays here; the classes give them the views of their pinned buffers."""
from __future__ import annotations

import itertools
import os

import numpy as np
import pytest

from ssd_amd.engine import logit_rules as LR
from ssd_amd.engine.sequence import Sequence
from ssd_amd.guide import TokenAutomaton
from ssd_amd.hip import constrain_ops as HC
from ssd_amd.sampling_params import SamplingParams
from tests import constrain_ref as CR
from tests import guide_ref as GR
from tests import penalty_ref as PR

V, K, EOS = 70, 3, 5        # V crosses a 32-bit mask word and is no multiple of 8
PROMPT = [7, 8, 9, 7, 40]
WORD16 = list(range(50, 66))        # a bad word of 16 tokens: its 15-token prefix fills the host tail exactly


def seq(sp, out, lookahead=None, prompt=PROMPT, guide=None):
    """A sequence with `out` generated and, behind it, the K entries a round's lookahead puts at the end of token_ids."""
    s = Sequence(list(prompt), sp, guide=guide)
    for t in list(out) + list(lookahead if lookahead is not None else [1, 2, 3]):
        s.append_token(t)
    return s


def rows_and_extra(B, rows_per_seq, seed):
    rng = np.random.default_rng(seed)
    bits = PR.f32_to_bf16(rng.normal(0, 3, size=(B * rows_per_seq, V + 2)).astype(np.float32))
    extra = rng.integers(0, V, size=(B, K + 1)) if rows_per_seq > 1 else None
    return bits, extra


# ---- penalties ---------------------------------------------------------------------------------------------------------------------
def penalty_arrays(B, L=64):
    return [np.zeros((B, L), np.int32), np.zeros((B, L), np.int32), np.zeros((B, L), np.float32), np.zeros(B, np.int32),
            np.zeros((3, B), np.float32)]


def penalty_batch():
    a = SamplingParams(repetition_penalty=1.3, presence_penalty=0.25, frequency_penalty=0.5, logit_bias={69: 2.5, 8: -1.0})   # 69: never in the history
    c = SamplingParams(frequency_penalty=-0.75)
    return [(seq(a, [40, 41, 41, 33]), a), (seq(SamplingParams(), [11, 12]), None), (seq(c, [9, 9, 20], lookahead=[-1, -1, -1]), c)]


def unpack_penalties(B, ids, cnt, bias, lens, par):
    tables = [[(int(ids[b, i]), int(cnt[b, i]) >> 1, int(cnt[b, i]) & 1, float(bias[b, i])) for i in range(lens[b])] for b in range(B)]
    return tables, par[0, :B], par[1, :B], par[2, :B]


@pytest.mark.parametrize("rows_per_seq", [1, K + 1])
def test_packed_penalties_are_the_history_counted_by_hand(rows_per_seq):
    batch = penalty_batch()
    arrays = penalty_arrays(len(batch))
    LR.pack_penalties([s for s, _ in batch], K, *arrays)
    tables, rep, pres, freq = unpack_penalties(len(batch), *arrays)
    want_tab, want_par = [], []
    for s, sp in batch:
        if sp is None:
            want_tab.append([])
            want_par.append((1.0, 0.0, 0.0))
            continue
        P, upto = len(PROMPT), len(s.token_ids) - K
        tab = PR.table_of(s.token_ids[:P], s.token_ids[P:upto], sp.logit_bias)
        want_tab.append([(t, c, ip, b) for t, (c, ip, b) in tab.items()])
        want_par.append((sp.repetition_penalty, sp.presence_penalty, sp.frequency_penalty))
    assert any(t == 69 and c == 0 and not ip for t, c, ip, _ in tables[0])         # the biased id that never occurred travels
    assert tables[1] == [] and len(tables[2]) == 5                                 # 7, 8, 9, 40 + 20: placeholders are no history
    bits, extra = rows_and_extra(len(batch), rows_per_seq, 1)
    got = PR.penalize_rows(bits, V, rows_per_seq, tables, rep, pres, freq, extra=extra)
    want = PR.penalize_rows(bits, V, rows_per_seq, want_tab, *np.array(want_par, np.float32).T, extra=extra)
    assert np.array_equal(got, want) and not np.array_equal(got, bits)


# ---- constraints -------------------------------------------------------------------------------------------------------------------
def constraint_arrays(B):
    return [np.zeros((B, HC.mask_words(V)), np.int32), np.zeros((B, HC.MAX_WORD_TOKENS), np.int32), np.zeros((B, HC.MAX_WORDS + 1), np.int32),
            np.zeros((B, HC.MAX_STOP), np.int32), np.zeros((B, HC.TAIL_LD), np.int32), np.zeros((5, B), np.int32)]


def constraint_batch():
    # a: the 15 tokens in front of the round are WORD16's prefix; min_tokens is met exactly at upto (15 output tokens)
    a = SamplingParams(min_tokens=15, stop_token_ids=[66, 67], allowed_token_ids=list(range(3, 69)), bad_words_ids=[[31], WORD16, [63, 12]])
    c = SamplingParams(min_tokens=6, stop_token_ids=[33], bad_words_ids=[[20, 21], [9, 20, 22]])
    return [(seq(a, WORD16[:15]), a), (seq(SamplingParams(), [11, 12]), None), (seq(c, [9, 9, 20], lookahead=[-1, -1, -1]), c)]


def unpack_constraints(B, bits, tok, off, stop, tail, par):
    out = []
    for b in range(B):
        words = [[int(t) for t in tok[b, off[b, w]:off[b, w + 1]]] for w in range(par[3, b])]
        out.append(dict(allow=bits[b].view(np.uint32) if par[0, b] else None, min_left=int(par[1, b]),
                        stops=[int(t) for t in stop[b, :par[2, b]]], words=words, tail=[int(t) for t in tail[b, :par[4, b]]]))
    return out


@pytest.mark.parametrize("rows_per_seq", [1, K + 1])
def test_packed_constraints_are_the_parameters_and_the_sliced_tail(rows_per_seq):
    batch = constraint_batch()
    arrays = constraint_arrays(len(batch))
    moved, any_words = LR.pack_constraints([s for s, _ in batch], K, V, EOS, [None] * 8, 0, *arrays)
    assert moved == [0] and any_words            # only the first sequence has a mask
    got_seqs = unpack_constraints(len(batch), *arrays)
    want_seqs = []
    for s, sp in batch:
        if sp is None:
            want_seqs.append({})
            continue
        P, upto = len(PROMPT), len(s.token_ids) - K
        want_seqs.append(dict(allow=CR.mask_of(sp.allowed_token_ids, V) if sp.allowed_token_ids is not None else None,
                              min_left=max(0, sp.min_tokens - (upto - P)), stops=list(sp.stop_token_ids) + [EOS],
                              words=sp.bad_words_ids, tail=s.token_ids[:upto]))
    assert got_seqs[0]["min_left"] == 0 and got_seqs[2]["min_left"] == 3 and len(got_seqs[0]["tail"]) == HC.TAIL_LD
    assert got_seqs[1] == dict(allow=None, min_left=0, stops=[], words=[], tail=[])
    bits, extra = rows_and_extra(len(batch), rows_per_seq, 2)
    got = CR.constrain_rows(bits, V, rows_per_seq, got_seqs, extra=extra)
    want = CR.constrain_rows(bits, V, rows_per_seq, want_seqs, extra=extra)
    assert np.array_equal(got, want)
    assert got[0, WORD16[15]] == CR.NINF and got[0, 31] == CR.NINF and got[0, 69] == CR.NINF and got[0, 12] != CR.NINF
    assert np.array_equal(got[rows_per_seq:2 * rows_per_seq], bits[rows_per_seq:2 * rows_per_seq])


# ---- guides ------------------------------------------------------------------------------------------------------------------------
def residues():
    """At state s every token t with t % 3 != s is allowed and leads to state t % 3."""
    return TokenAutomaton(3, 0, {s: {t: t % 3 for t in range(V) if t % 3 != s} for s in range(3)})


def guide_batch():
    sp = SamplingParams(guided_automaton=residues())
    return [(seq(sp, [1, 2, 4, 5]), sp), (seq(SamplingParams(), [11, 12]), None), (seq(sp, [2, 1], lookahead=[-1, -1, -1]), sp),
            (seq(sp, [1, 4, 2]), sp)]        # the last one broke its guide (4 at state 1): its state is -1


@pytest.mark.parametrize("rows_per_seq", [1, K + 1])
def test_packed_guides_are_the_states_walked_by_delta(rows_per_seq):
    batch = guide_batch()
    B = len(batch)
    par = np.zeros((3, B), np.int32)
    moved = LR.pack_guides([s for s, _ in batch], K, [None] * 8, 0, par)
    assert moved == [0, 2, 3]
    want_on, want_s0, autos = [], [], []
    for s, sp in batch:
        a = sp.guided_automaton if sp is not None else None
        st = a.start if a is not None else 0
        for t in (s.token_ids[len(PROMPT):len(s.token_ids) - K] if a is not None else []):
            st = a.delta(st, t)
        want_on.append(int(a is not None))
        want_s0.append(st)
        autos.append(GR.tables_of(a) if a is not None else None)
    assert want_s0 == [2, 0, 1, -1]
    assert [int(x) for x in par[2]] == [3, 0, 3, 3]
    bits, extra = rows_and_extra(B, rows_per_seq, 3)
    T = B * rows_per_seq
    got = GR.guide_rows(bits, V, rows_per_seq, autos, GR.walk(T, rows_per_seq, autos, par[0], par[1], extra=extra))
    want = GR.guide_rows(bits, V, rows_per_seq, autos, GR.walk(T, rows_per_seq, autos, want_on, want_s0, extra=extra))
    assert np.array_equal(got, want) and not np.array_equal(got[:rows_per_seq], bits[:rows_per_seq])
    for b in (1, 3):            # no guide, and a guide that was left: untouched
        assert np.array_equal(got[b * rows_per_seq:(b + 1) * rows_per_seq], bits[b * rows_per_seq:(b + 1) * rows_per_seq])


# ---- stale rows, limits, slots -----------------------------------------------------------------------------------------------------
def test_a_row_whose_new_sequence_has_no_rule_reads_as_off():
    plain = seq(SamplingParams(), [11, 12])
    pen, con, gd = penalty_batch(), constraint_batch(), guide_batch()
    arrays = penalty_arrays(3)
    LR.pack_penalties([pen[0][0], pen[2][0], pen[1][0]], K, *arrays)
    assert arrays[3][1] > 0
    LR.pack_penalties([pen[0][0], plain, pen[2][0]], K, *arrays)
    assert arrays[3][1] == 0 and [float(x) for x in arrays[4][:, 1]] == [1.0, 0.0, 0.0]
    arrays = constraint_arrays(3)
    LR.pack_constraints([con[0][0], con[2][0], con[1][0]], K, V, EOS, [None] * 3, 0, *arrays)
    assert arrays[5][:, 1].any()
    LR.pack_constraints([con[0][0], plain, con[2][0]], K, V, EOS, [None] * 3, 0, *arrays)
    assert not arrays[5][:, 1].any() and arrays[5][:, 2].any()
    par = np.zeros((3, 3), np.int32)
    LR.pack_guides([gd[0][0], gd[2][0], gd[1][0]], K, [None] * 3, 0, par)
    assert par[0, 1] == 1
    LR.pack_guides([gd[0][0], plain, gd[2][0]], K, [None] * 3, 0, par)
    assert par[0, 1] == 0 and not par[:, 1].any() and par[0, 2] == 1


def test_the_limits_are_still_refused_with_their_texts():
    s = seq(SamplingParams(repetition_penalty=1.2), [40, 41, 42])
    with pytest.raises(ValueError, match=rf"the history of sequence {s.seq_id} \(9 distinct token and logit_bias ids\) does not fit the "
                                         r"penalty table of 4 entries \(max_model_len \+ 1024\)"):
        LR.pack_penalties([s], 0, *penalty_arrays(1, L=4))
    s = seq(SamplingParams(min_tokens=2, stop_token_ids=list(range(6, 70))), [40])
    with pytest.raises(ValueError, match=rf"sequence {s.seq_id} has 65 stop ids \(the EOS included\) to hold back under min_tokens: "
                                         r"at most 64"):
        LR.pack_constraints([s], 0, V, EOS, [None], 0, *constraint_arrays(1))


def test_a_table_travels_when_its_sequence_takes_a_slot_it_did_not_have():
    cap = 8
    owner = [None] * cap
    assert LR.take_slots(owner, [10, None, 12]) == [0, 2] and owner[:3] == [10, None, 12]
    assert LR.take_slots(owner, [10, None, 12]) == []                   # kept their slots: nothing is sent again
    assert LR.take_slots(owner, [12, 10]) == [0, 1]                     # moved: both are sent
    assert LR.take_slots(owner, [20, 21], base=cap - 2) == [0, 1]       # a prefill of two arrivals uses the last slots ...
    assert owner[:2] == [12, 10] and owner[cap - 2:] == [20, 21]        # ... and leaves slot 0 to the running sequence
    assert LR.take_slots(owner, [12, 10]) == []
    assert LR.take_slots(owner, [20]) == [0] and LR.take_slots(owner, [12]) == [0]      # taken over, then the old owner returns: sent again


# ---- Sampling ----------------------------------------------------------------------------------------------------------------------
def test_sampled_verify_graphs_are_the_names_that_start_with_verify_s():
    from ssd_amd.engine.model_runner import Sampling
    on_off = (False, True)
    # what ModelRunner.verify_chain enumerated before it tested the name
    baked = {"verify" + Sampling(True, f, p, l, d, c, g).suffix for f in on_off for p in on_off for l in on_off for d in on_off
             for c in on_off for g in on_off}
    assert len(baked) == 64 and not "verify_logits".startswith("verify_s") and "verify_logits" not in baked
    for fields in itertools.product(on_off, repeat=7):
        how = Sampling(*fields)
        name = "verify" + how.suffix
        assert name.startswith("verify_s") == (name in baked), fields
        if how.sample or not how.filt:      # (a filter without a temperature is never built, and its name is the sampled one's)
            assert name.startswith("verify_s") == how.sample, fields
        assert how.adjusts == (how.pen or how.con or how.gd)


# ---- bind --------------------------------------------------------------------------------------------------------------------------
def test_bind_names_the_symbol_the_library_does_not_export():
    import ctypes as C
    from ssd_amd.hip.lib import SsdHipError, bind, build_library, lib_path
    if not os.path.exists(lib_path()):
        build_library()
    with pytest.raises(SsdHipError, match="libssdhip.so does not export ssd_no_such_rule"):
        bind({"ssd_abi_version": [], "ssd_no_such_rule": [C.c_void_p, C.c_int]})
    table = {"ssd_abi_version": []}
    assert bind(table) is bind(table) and bind(table).ssd_abi_version.restype is C.c_int

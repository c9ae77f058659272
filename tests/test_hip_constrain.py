"""ssd_constrain_rows (csrc/constrain.hip, include/ssd_hip_constrain.h) on the GPU against tests/constrain_ref.py: every case compares
BITS over the whole [T][ld] buffer, pad columns (a NaN sentinel) included.

Shapes: V = 1000 / ld = 1024 (one slice, the last mask word 8 bits wide), V = 4136 / ld = 4160 (two slices, the second 40 entries, a
partial last word), V = 1003 / ld = 1011 (rows that are not 16-byte aligned, a last chunk cut by V), and one case at V = 128256 with two
rows.  T = 1, T = 5 with rows_per_seq = 5 (prefix form: row j sees exactly j extras) and B = 3 with a sequence that has everything off
between two constrained ones.  The special values +-0, +-inf and two NaNs are planted at banned and at kept entries of every row; every
list carries the ids -1, V and ld - 1, which ban nothing (nothing is written at or past V: the sentinel survives); the unused parts of
every device buffer hold poison, the bits at and past V of the last mask word included."""
import numpy as np
import pytest
import torch

from tests import constrain_ref as R

pytestmark = pytest.mark.gpu

SHAPES = [(1000, 1024), (4136, 4160), (1003, 1011)]
SENTINEL = 0x7FC5
SPECIAL = [0x0000, 0x8000, 0x7F80, 0xFF80, 0x7FC1, 0xFFC0]          # +0 -0 +inf -inf NaN NaN
TAIL_LD = 15
RULES = ["allow", "min", "words", "all"]


@pytest.fixture(scope="module")
def C():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ssd_amd.hip import constrain_ops
    constrain_ops.load_constrain_library()
    return constrain_ops


def make_rows(rng, T, V, ld):
    x = torch.from_numpy(rng.standard_normal((T, ld)).astype(np.float32) * 4).to(torch.bfloat16)
    bits = x.view(torch.int16).numpy().view(np.uint16).copy()
    bits[:, V:] = SENTINEL
    return bits


def to_dev(bits):
    return torch.from_numpy(bits.view(np.int16).copy()).cuda().view(torch.bfloat16)


def to_bits(d):
    return d.cpu().view(torch.int16).numpy().view(np.uint16)


def i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()


def device_lists(C, seqs, V, high_bits: int = 0xFFFFFFFF):
    """The device buffers of every group from the per-sequence dicts of constrain_ref.constrain_rows.  Unused parts hold poison: ids
    that would ban something if they were read, mask bits at and past V set (high_bits) in the last word."""
    B, W = len(seqs), C.mask_words(V)
    on = np.zeros(B, np.int32)
    bits = np.zeros((B, W), np.uint32)              # an off sequence's mask allows nothing: it must not be read as one
    min_left = np.full(B, 99, np.int32)             # ... and so on: an off sequence has stop_len 0, bw_n 0
    stop = np.full((B, C.MAX_STOP), 3, np.int32)
    stop_len = np.zeros(B, np.int32)
    tok = np.full((B, C.MAX_WORD_TOKENS), 5, np.int32)
    off = np.zeros((B, C.MAX_WORDS + 1), np.int32)
    bw_n = np.zeros(B, np.int32)
    tail = np.full((B, TAIL_LD), 5, np.int32)
    tail_len = np.zeros(B, np.int32)
    for b, s in enumerate(seqs):
        if s.get("allow") is not None:
            on[b] = 1
            bits[b] = s["allow"]
            if V % 32:
                bits[b, -1] |= np.uint32(high_bits & ~((1 << (V % 32)) - 1) & 0xFFFFFFFF)
        min_left[b] = s.get("min_left", 0)
        st = list(s.get("stops", ()))
        stop[b, :len(st)] = st
        stop_len[b] = len(st)
        flat, offs = R.flatten_words(s.get("words", ()))
        tok[b, :len(flat)] = flat
        off[b, :len(offs)] = offs
        off[b, len(offs):] = 7                      # poison behind the used offsets
        bw_n[b] = len(s.get("words", ()))
        t = list(s.get("tail", ()))[-TAIL_LD:]
        tail[b, :len(t)] = t
        tail_len[b] = len(t)
    return dict(allow_on=i32(on), allow_bits=torch.from_numpy(bits.view(np.int32).copy()).cuda(), min_left=i32(min_left), stop_ids=i32(stop),
                stop_len=i32(stop_len), bw_tok=i32(tok), bw_off=i32(off), bw_n=i32(bw_n), tail=i32(tail), tail_ld=TAIL_LD,
                tail_len=i32(tail_len))


def run(C, bits, V, rows_per_seq, seqs, extra=None, extra_n=None, **kw):
    T, ld = bits.shape
    d = to_dev(bits)
    lists = device_lists(C, seqs, V, **kw)
    if extra is not None:
        ex = torch.tensor(extra, dtype=torch.int64, device="cuda")
        lists.update(extra=ex, extra_ld=ex.shape[1], extra_n=None if extra_n is None else torch.tensor([extra_n], dtype=torch.int32, device="cuda"))
    C.constrain_rows(d, ld, T, V, rows_per_seq, **lists)
    torch.cuda.synchronize()
    return to_bits(d)


def plant_specials(rng, bits, V, rows_per_seq, seqs, extra=None, extra_n=None):
    """SPECIAL at six banned and six kept entries of every row that has both (found with the reference: it only decides where)."""
    probe = R.constrain_rows(np.zeros_like(bits), V, rows_per_seq, seqs, extra, extra_n)
    for r in range(bits.shape[0]):
        ban = np.nonzero(probe[r, :V] == R.NINF)[0]
        keep = np.nonzero(probe[r, :V] != R.NINF)[0]
        for pool in (ban, keep):
            if len(pool):
                for v, t in zip(SPECIAL, rng.permutation(pool)[:len(SPECIAL)]):
                    bits[r, t] = v


def check(C, bits, V, rows_per_seq, seqs, extra=None, extra_n=None, **kw):
    got = run(C, bits, V, rows_per_seq, seqs, extra, extra_n, **kw)
    want = R.constrain_rows(bits, V, rows_per_seq, seqs, extra, extra_n)
    bad = np.argwhere(got != want)
    assert bad.size == 0, [(int(r), int(c), hex(bits[r, c]), hex(got[r, c]), hex(want[r, c])) for r, c in bad[:8]]
    assert (got[:, V:] == SENTINEL).all()
    # the normative text once more, without the reference: only -inf is ever written, and only below V
    changed = got != bits
    assert (got[changed] == R.NINF).all()
    return got


def scenario(rng, V, ld, rows_per_seq, rule, min_left=2, tail_len=TAIL_LD):
    """One constrained sequence and its extras row [rows_per_seq] (entry 0 = the tail's last token).  words: one, two and sixteen tokens
    long, matching wholly in the tail (row 0), wholly in the extras (row 2), across the boundary (rows 1 and 3), never (a prefix that
    does not occur, a word longer than the context when the tail is short), two words and the mask banning the same token."""
    tail = [int(t) for t in rng.integers(0, V, size=tail_len)]
    ex = [tail[-1]] + [int(t) for t in rng.integers(0, V, size=rows_per_seq - 1)]
    s = dict(tail=tail)
    fresh = iter(int(t) for t in rng.permutation(V) if t not in tail and t not in ex)
    twice = next(fresh)
    mark = s["mark"] = {}          # name -> (last token of a word, the rows it is banned in); the reference ignores the key
    if rule in ("allow", "all"):
        allowed = [int(t) for t in rng.choice(V, size=max(8, V // 3), replace=False) if t != twice] + [-1, V, ld - 1, V - 1]
        s["allow"] = R.mask_of(allowed, V)
        s["twice"] = twice
    if rule in ("min", "all"):
        s["min_left"] = min_left
        s["stops"] = [next(fresh) for _ in range(5)] + [-1, V, ld - 1, 0, V - 1]
    if rule in ("words", "all"):
        mark["tail2"], mark["tail16"], mark["never"] = (next(fresh), [0]), (next(fresh), [0]), (next(fresh), [])
        w = [[next(fresh)], [twice], [tail[-1], twice],                         # one token; the same last token twice (and masked)
             [tail[-1], mark["tail2"][0]],                                      # two tokens, in the tail: row 0
             [-1], [V], [ld - 1], [tail[-1], V], [V, next(fresh)], [tail[-1], -1],      # out-of-range ids ban nothing
             [next(fresh), next(fresh)]]                                        # a prefix that does not end the context
        if len(tail) == TAIL_LD:
            w.append(tail[-15:] + [mark["tail16"][0]])                          # sixteen tokens, wholly in the tail: row 0
            w.append([next(fresh)] + tail[-14:] + [mark["never"][0]])           # ... whose first token is wrong: never
        else:
            del mark["tail16"]
            w.append([next(fresh)] * 2 + tail + [mark["never"][0]])             # longer than the context of row 0 (its end would match)
        if rows_per_seq >= 3:
            mark["extras2"], mark["across3"] = (next(fresh), [2]), (next(fresh), [1])
            w.append([ex[2], mark["extras2"][0]])                               # two tokens, wholly in the extras: row 2
            w.append([tail[-1], ex[1], mark["across3"][0]])                     # across the boundary: row 1
        if rows_per_seq >= 4 and len(tail) == TAIL_LD:
            mark["across16"] = (next(fresh), [3])
            w.append(tail[-12:] + ex[1:4] + [mark["across16"][0]])              # sixteen tokens across the boundary: row 3
        s["words"] = w
        if "allow" in s:            # the marked tokens are allowed: what bans them is their word
            s["allow"] |= R.mask_of([t for t, _ in mark.values()], V)
    return s, ex


def check_marks(got, bits, s, row0=0, rows=1):
    """Every marked word bans its last token in exactly the rows it matches in; elsewhere the entry keeps its bits."""
    for name, (t, where) in s["mark"].items():
        for j in range(rows):
            assert got[row0 + j, t] == (R.NINF if j in where else bits[row0 + j, t]), (name, j)


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("V,ld", SHAPES)
def test_one_row_five_rows_and_three_sequences(C, V, ld, rule):
    rng = np.random.default_rng(100 * V + RULES.index(rule))
    # T = 1
    s, ex = scenario(rng, V, ld, 1, rule)
    bits = make_rows(rng, 1, V, ld)
    plant_specials(rng, bits, V, 1, [s])
    got = check(C, bits, V, 1, [s])
    assert (got != bits).any()
    check_marks(got, bits, s)
    # T = 5, rows_per_seq = 5: row j sees exactly j extras
    rps = 5
    s, ex = scenario(rng, V, ld, rps, rule)
    bits = make_rows(rng, rps, V, ld)
    plant_specials(rng, bits, V, rps, [s], [ex])
    got = check(C, bits, V, rps, [s], [ex])
    check_marks(got, bits, s, 0, rps)       # the rows differ in what the words ban: the extras are seen row by row
    assert rule not in ("words", "all") or len(s["mark"]) == 6
    # B = 3: everything off in the middle, its rows on special values and its lists full of poison
    seqs, extra = [], []
    for b in range(3):
        s, ex = scenario(rng, V, ld, rps, rule, min_left=(0, 2, rps + 3)[b])
        seqs.append(s if b != 1 else dict(tail=s["tail"]))
        extra.append(ex)
    bits = make_rows(rng, 3 * rps, V, ld)
    plant_specials(rng, bits, V, rps, seqs, extra)
    bits[rps:2 * rps, :len(SPECIAL)] = SPECIAL
    got = check(C, bits, V, rps, seqs, extra)
    assert (got[rps:2 * rps] == bits[rps:2 * rps]).all()
    assert (got[2 * rps:] != bits[2 * rps:]).any()
    check_marks(got, bits, seqs[0], 0, rps)
    check_marks(got, bits, seqs[2], 2 * rps, rps)
    # the bits at and past V in the last mask word are ignored whatever they hold
    assert (run(C, bits, V, rps, seqs, extra, high_bits=0) == got).all()


@pytest.mark.parametrize("V,ld", SHAPES)
def test_min_left_zero_two_and_more_than_the_rows(C, V, ld):
    rng = np.random.default_rng(V + 7)
    rps = 5
    stops = [3, V - 1, 4097 % V, -1, V, ld - 1]
    seqs = [dict(min_left=m, stops=stops) for m in (0, 2, rps + 4)]
    extra = [[int(t) for t in rng.integers(0, V, size=rps)] for _ in seqs]
    bits = make_rows(rng, 3 * rps, V, ld)
    plant_specials(rng, bits, V, rps, seqs, extra)
    got = check(C, bits, V, rps, seqs, extra)
    banned = (got[:, 3] == R.NINF) & (got[:, V - 1] == R.NINF) & (got[:, 4097 % V] == R.NINF)
    assert banned.tolist() == [False] * rps + [True, True, False, False, False] + [True] * rps
    assert (got[:rps] == bits[:rps]).all()


@pytest.mark.parametrize("V,ld", SHAPES)
def test_a_word_longer_than_the_context_and_one_token_banned_three_times(C, V, ld):
    rng = np.random.default_rng(V + 9)
    s, ex = scenario(rng, V, ld, 1, "all", tail_len=2)
    bits = make_rows(rng, 1, V, ld)
    plant_specials(rng, bits, V, 1, [s])
    got = check(C, bits, V, 1, [s])
    twice = s["twice"]
    assert got[0, twice] == R.NINF and "tail16" not in s["mark"]
    check_marks(got, bits, s)
    # an empty tail: only one-token words can match
    s2 = dict(s, tail=[])
    got = check(C, bits, V, 1, [s2])
    assert got[0, twice] == R.NINF and got[0, s["mark"]["tail2"][0]] == bits[0, s["mark"]["tail2"][0]]


def test_the_llama_vocabulary_with_two_rows(C):
    V = ld = 128256
    rng = np.random.default_rng(5)
    s, ex = scenario(rng, V, ld, 2, "all")
    s["words"].append([s["tail"][-1], ex[1], V - 1])          # across the boundary, the last entry of the last slice: row 1
    bits = make_rows(rng, 2, V, ld)
    plant_specials(rng, bits, V, 2, [s], [ex])
    got = check(C, bits, V, 2, [s], [ex])
    assert got[1, V - 1] == R.NINF
    # sparse lists alone: everything but a handful of entries keeps its bits
    s2 = {k: v for k, v in s.items() if k != "allow"}
    got = check(C, bits, V, 2, [s2], [ex])
    assert 0 < (got != bits).sum() < 40
    # a mask of eight ids
    s3 = dict(allow=R.mask_of([0, 31, 32, 4095, 4096, 70000, V - 2, V - 1], V))
    got = check(C, bits, V, 2, [s3])
    assert ((got[:, :V] != R.NINF).sum(axis=1) <= 8).all()


def test_chain_form_follows_extra_n_between_replays_of_one_graph(C):
    """One capture; the step counter, the mask and the tail are rewritten in device memory between the replays."""
    from ssd_amd.utils.graphs import capture
    V, ld = SHAPES[1]
    rng = np.random.default_rng(23)
    B, E = 3, 17                    # 16 extras: a sixteen-token word can lie wholly in them
    seqs, extra = [], []
    for b in range(B):
        s, _ = scenario(rng, V, ld, 1, "all", min_left=(1, 3, 40)[b])
        ex = [s["tail"][-1]] + [int(t) for t in rng.integers(0, V, size=E - 1)]
        # last tokens that nothing else bans, and that the mask allows: in the extras, across the boundary, sixteen in the extras
        free = [t for t in range(40, V) if (int(s["allow"][t >> 5]) >> (t & 31)) & 1 and t not in R.banned(V, [], 0, None, 99, s["stops"], [[w[-1]] for w in s["words"]])]
        s["m"] = free[:3]
        s["words"] += [[ex[3], free[0]], [s["tail"][-1], ex[1], ex[2], ex[3], free[1]], ex[1:16] + [free[2]]]
        seqs.append(s)
        extra.append(ex)
    seqs[1] = dict(tail=seqs[1]["tail"])            # everything off in the middle
    bits = make_rows(rng, B, V, ld)
    lists = device_lists(C, seqs, V)
    exd = torch.tensor(extra, dtype=torch.int64, device="cuda")
    step = torch.zeros(1, dtype=torch.int32, device="cuda")
    static = to_dev(bits)
    graph, stream = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with capture(graph, stream=stream):
        C.constrain_rows(static, ld, B, V, 1, **lists, extra=exd, extra_ld=E, extra_n=step)
    seen = {}
    for n in (0, 3, E + 4, 15, -2):          # past E - 1 the counter is clamped, below 0 it is 0
        static.copy_(to_dev(bits))
        step.fill_(n)
        graph.replay()
        torch.cuda.synchronize()
        got = to_bits(static)
        want = R.constrain_rows(bits, V, 1, seqs, extra, n)
        assert (got == want).all(), n
        assert (got[:, V:] == SENTINEL).all() and (got[1] == bits[1]).all()
        assert (run(C, bits, V, 1, seqs, extra, n) == got).all()          # the eager launch with the same counter: the same bits
        seen[n] = got.copy()
    for b in (0, 2):
        m = seqs[b]["m"]
        assert [seen[0][b, t] == bits[b, t] for t in m] == [True] * 3
        assert [seen[3][b, t] == R.NINF for t in m] == [True, True, False]          # wholly in the extras; across the boundary
        assert [seen[15][b, t] == R.NINF for t in m] == [False, False, True]        # sixteen tokens wholly in the extras
    assert (seen[-2] == seen[0]).all() and not (seen[0] == seen[3]).all()
    assert (seen[E + 4] == R.constrain_rows(bits, V, 1, seqs, extra, E - 1)).all()
    # min_left 1 / 40: one extra lifts the first sequence's stop ban, nothing lifts the third's
    st0, st2 = seqs[0]["stops"][0], seqs[2]["stops"][0]
    assert seen[0][0, st0] == R.NINF and seen[3][2, st2] == R.NINF and seen[15][2, st2] == R.NINF
    # fresh data under the same graph: another mask and another tail for sequence 0, sequence 1 switched on
    seqs2 = [dict(seqs[0]), dict(seqs[0]), seqs[2]]
    seqs2[0]["allow"] = R.mask_of(range(0, V, 3), V)
    seqs2[0]["tail"] = seqs[2]["tail"]
    fresh = device_lists(C, seqs2, V)
    for k, v in lists.items():
        if torch.is_tensor(v):
            v.copy_(fresh[k])
    static.copy_(to_dev(bits))
    step.fill_(3)
    graph.replay()
    torch.cuda.synchronize()
    got = to_bits(static)
    assert (got == R.constrain_rows(bits, V, 1, seqs2, extra, 3)).all()
    assert (got[1] != bits[1]).any() and not (got[0] == seen[3][0]).all()


def test_two_runs_of_the_same_input_are_bit_identical(C):
    V, ld = SHAPES[1]
    rng = np.random.default_rng(11)
    rps = 5
    seqs, extra = zip(*(scenario(rng, V, ld, rps, "all") for _ in range(3)))
    bits = make_rows(rng, 3 * rps, V, ld)
    plant_specials(rng, bits, V, rps, seqs, extra)
    a = check(C, bits, V, rps, list(seqs), list(extra))
    b = run(C, bits, V, rps, list(seqs), list(extra))
    assert (a == b).all()


def test_null_groups_switch_a_rule_off(C):
    V, ld = SHAPES[0]
    rng = np.random.default_rng(3)
    s, ex = scenario(rng, V, ld, 5, "all")
    bits = make_rows(rng, 5, V, ld)
    lists = device_lists(C, [s], V)
    groups = dict(allow=("allow_on", "allow_bits"), min=("min_left", "stop_ids", "stop_len"), words=("bw_tok", "bw_off", "bw_n", "tail", "tail_len"))
    exd = torch.tensor([ex], dtype=torch.int64, device="cuda")
    for drop in (("allow",), ("min",), ("words",), ("allow", "min"), ("allow", "min", "words")):
        kw = {k: (None if any(k in groups[g] for g in drop) else v) for k, v in lists.items()}
        d = to_dev(bits)
        C.constrain_rows(d, ld, 5, V, 5, **kw, extra=exd, extra_ld=5)
        torch.cuda.synchronize()
        s2 = dict(s)
        for g in drop:
            for key in dict(allow=("allow",), min=("min_left", "stops"), words=("words",))[g]:
                s2.pop(key)
        assert (to_bits(d) == R.constrain_rows(bits, V, 5, [s2], [ex])).all(), drop
    d = to_dev(bits)
    C.constrain_rows(d, ld, 5, V, 5, **lists)          # no extras: every row is row 0
    torch.cuda.synchronize()
    assert (to_bits(d) == R.constrain_rows(bits, V, 5, [s], None)).all()


def test_each_refusal_code(C):
    import ctypes as CT
    lib = C.load_constrain_library()
    x = torch.zeros(2, 16, dtype=torch.bfloat16, device="cuda")
    i = torch.zeros(2, 2048, dtype=torch.int32, device="cuda")
    ex = torch.zeros(2, 4, dtype=torch.int64, device="cuda")
    n = torch.zeros(2, dtype=torch.int32, device="cuda")
    p = lambda t: None if t is None else CT.c_void_p(t.data_ptr())
    good = dict(logits=x, ld=16, T=2, V=16, rps=1, allow_on=n, allow_bits=i, min_left=n, stop_ids=i, stop_len=n, bw_tok=i, bw_off=i, bw_n=n,
                tail=i, tail_ld=15, tail_len=n, extra=None, extra_ld=0, extra_n=None)

    def call(**kw):
        a = dict(good, **kw)
        return lib.ssd_constrain_rows(p(a["logits"]), a["ld"], a["T"], a["V"], a["rps"], p(a["allow_on"]), p(a["allow_bits"]),
                                      p(a["min_left"]), p(a["stop_ids"]), p(a["stop_len"]), p(a["bw_tok"]), p(a["bw_off"]), p(a["bw_n"]),
                                      p(a["tail"]), a["tail_ld"], p(a["tail_len"]), p(a["extra"]), a["extra_ld"], p(a["extra_n"]), None)
    SHAPE, ARG = -1, -3          # SSD_ERR_SHAPE, SSD_ERR_ARG (include/ssd_hip.h)
    for kw in (dict(T=0), dict(T=-1), dict(T=65536), dict(V=0), dict(rps=0), dict(ld=8), dict(tail_ld=0), dict(tail_ld=16),
               dict(extra=ex, extra_ld=0), dict(extra=ex, extra_ld=C.MAX_EXTRA + 2, extra_n=n), dict(extra=ex, extra_ld=4, rps=5)):
        assert call(**kw) == SHAPE, kw
    for kw in (dict(logits=None), dict(allow_on=None), dict(allow_bits=None), dict(min_left=None), dict(stop_ids=None), dict(stop_len=None),
               dict(bw_tok=None), dict(bw_off=None), dict(bw_n=None), dict(tail=None), dict(tail_len=None), dict(extra_n=n)):
        assert call(**kw) == ARG, kw
    assert call() == 0
    none = dict(allow_on=None, allow_bits=None, min_left=None, stop_ids=None, stop_len=None, bw_tok=None, bw_off=None, bw_n=None, tail=None,
                tail_len=None)
    assert call(**none) == 0 and call(**none, tail_ld=0) == 0          # null groups are "off"; tail_ld only counts with bad words
    assert call(extra=ex, extra_ld=4, rps=2) == 0 and call(extra=ex, extra_ld=4, extra_n=n) == 0
    torch.cuda.synchronize()
    assert (x == 0).all()          # everything off (allow_on 0, stop_len 0, bw_n 0): nothing was written
    from ssd_amd.hip.lib import SsdHipError
    with pytest.raises(SsdHipError, match="ssd_constrain_rows"):
        C.constrain_rows(x, 8, 2, 16, 1)

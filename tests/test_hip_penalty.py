"""ssd_penalize_rows (csrc/penalty.hip, include/ssd_hip_penalty.h) on the GPU against tests/penalty_ref.py: every case compares BITS over
the whole [T][ld] buffer, pad columns (a NaN sentinel) included.

Shapes: V = 1000 / ld = 1024 and V = 2500 / ld = 2560 (V no multiple of anything, ld > V); T = 1, T = 5 with rows_per_seq = 5, and
B = 3 sequences whose tables hold 0, 1 and tab_ld entries.  The logits at the first table ids are +0.0, -0.0, +inf, -inf, two NaNs, a
positive and a negative value; tables and extras carry the ids -1, V and ld - 1, which must be ignored (nothing is written at or past
V: the sentinel survives)."""
import numpy as np
import pytest
import torch

from tests import penalty_ref as R

pytestmark = pytest.mark.gpu

SHAPES = [(1000, 1024), (2500, 2560)]
TAB_LD = 48
SENTINEL = 0x7FC5
SPECIAL = [0x0000, 0x8000, 0x7F80, 0xFF80, 0x7FC1, 0xFFC0, 0x4049, 0xC049]          # +0 -0 +inf -inf NaN NaN 3.14 -3.14
PARAMS = {                                  # (r, p, f, with bias)
    "repetition": (1.3, 0.0, 0.0, False),
    "presence": (1.0, 0.75, 0.0, False),
    "frequency": (1.0, 0.0, 0.3, False),
    "bias": (1.0, 0.0, 0.0, True),
    "all_four": (1.2, 0.5, 0.25, True),
    "r_below_1": (0.7, 0.0, 0.0, False),
    "negative_p_f": (1.0, -0.6, -0.2, True),
}


@pytest.fixture(scope="module")
def P():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ssd_amd.hip import penalty_ops
    penalty_ops.load_penalty_library()
    return penalty_ops


def make_rows(rng, T, V, ld):
    x = torch.from_numpy(rng.standard_normal((T, ld)).astype(np.float32) * 4).to(torch.bfloat16)
    bits = x.view(torch.int16).numpy().view(np.uint16).copy()
    bits[:, V:] = SENTINEL
    return bits


def make_table(rng, V, ld, n, bias: bool):
    """n entries (id, count, in_prompt, bias) with unique ids; from 4 entries on, three of them are the ids -1, V and ld - 1.  Both
    kinds of biased entry occur: unseen (count 0, not in the prompt) and seen."""
    ids = [int(t) for t in rng.choice(V, size=n, replace=False)]
    if n >= 4:
        ids[1], ids[2], ids[3] = -1, V, ld - 1
    tab = []
    for i, t in enumerate(ids):
        c, ip = int(rng.integers(0, 4)), bool(rng.integers(0, 2))
        b = float(rng.choice([0.0, 1.5, -2.25, 100.0, -100.0])) if bias else 0.0
        if bias and i % 5 == 0:
            c, ip, b = 0, False, 7.5          # a bias on an unseen token
        if bias and i % 5 == 4:
            c, ip, b = 2, True, -7.5          # a bias on a seen one
        tab.append((t, c, ip, b))
    return tab


def plant_specials(bits, tables, rows_per_seq, V):
    """The special logit values go where the arithmetic happens: at the valid ids of each sequence's table, in every row of it."""
    for b, tab in enumerate(tables):
        valid = [t for t, *_ in tab if 0 <= t < V]
        for i, t in enumerate(valid[:len(SPECIAL)] if len(valid) > 1 else []):
            bits[b * rows_per_seq:(b + 1) * rows_per_seq, t] = SPECIAL[i]


def device_tables(P, tables, tab_ld):
    """Device tensors of the tables; the unused tail of every table row is poison that must not be read as history."""
    B = len(tables)
    ids = torch.full((B, tab_ld), 3, dtype=torch.int32)
    cnt = torch.full((B, tab_ld), P.pack_count(9, True), dtype=torch.int32)
    bias = torch.full((B, tab_ld), 55.0, dtype=torch.float32)
    lens = torch.zeros(B, dtype=torch.int32)
    for b, tab in enumerate(tables):
        lens[b] = len(tab)
        for i, (t, c, ip, bs) in enumerate(tab):
            ids[b, i], cnt[b, i], bias[b, i] = t, P.pack_count(c, ip), bs
    return ids.cuda(), cnt.cuda(), bias.cuda(), lens.cuda()


def f32(v):
    return torch.tensor(v, dtype=torch.float32, device="cuda")


def to_dev(bits):
    return torch.from_numpy(bits.view(np.int16).copy()).cuda().view(torch.bfloat16)


def to_bits(d):
    return d.cpu().view(torch.int16).numpy().view(np.uint16)


def run(P, bits, V, rows_per_seq, tables, rep, pres, freq, extra=None, extra_n=None, tab_ld=TAB_LD):
    T, ld = bits.shape
    d = to_dev(bits)
    tabs = device_tables(P, tables, tab_ld) if tables is not None else (None, None, None, None)
    kw = {}
    if extra is not None:
        ex = torch.tensor(extra, dtype=torch.int64, device="cuda")
        kw = dict(extra=ex, extra_ld=ex.shape[1], extra_n=None if extra_n is None else torch.tensor([extra_n], dtype=torch.int32, device="cuda"))
    P.penalize_rows(d, ld, T, V, rows_per_seq, tabs[0], tabs[1], tabs[2], tab_ld, tabs[3], f32(rep), f32(pres), f32(freq), **kw)
    torch.cuda.synchronize()
    return to_bits(d)


def check(P, bits, V, rows_per_seq, tables, rep, pres, freq, extra=None, extra_n=None, tab_ld=TAB_LD):
    got = run(P, bits, V, rows_per_seq, tables, rep, pres, freq, extra, extra_n, tab_ld)
    want = R.penalize_rows(bits, V, rows_per_seq, tables, rep, pres, freq, extra, extra_n)
    bad = np.argwhere(got != want)
    assert bad.size == 0, [(int(r), int(c), hex(bits[r, c]), hex(got[r, c]), hex(want[r, c])) for r, c in bad[:8]]
    assert (got[:, V:] == SENTINEL).all()
    return got


def extras_for(rng, tables, V, ld, n_extra):
    """[B][1 + n_extra]: entry 0 is the round's first input (not an extra); the rest repeat each other, hit the table, are new, or
    are out of range."""
    out = []
    for tab in tables:
        valid = [t for t, *_ in tab if 0 <= t < V]
        new = int(rng.integers(0, V))
        pool = [new, new, -1, V, ld - 1, int(rng.integers(0, V))] + valid[:3] + valid[:1]
        row = [int(rng.integers(0, V))] + [int(pool[i]) for i in rng.permutation(len(pool))[:n_extra]]
        out.append(row + [new] * (1 + n_extra - len(row)))
    return out


@pytest.mark.parametrize("name", list(PARAMS))
@pytest.mark.parametrize("V,ld", SHAPES)
def test_table_only_one_row_and_three_sequences(P, V, ld, name):
    r, p, f, bias = PARAMS[name]
    rng = np.random.default_rng(100 * V + list(PARAMS).index(name))
    # T = 1
    tables = [make_table(rng, V, ld, 12, bias)]
    bits = make_rows(rng, 1, V, ld)
    plant_specials(bits, tables, 1, V)
    got = check(P, bits, V, 1, tables, [r], [p], [f])
    assert (got != bits).any(), "the case adjusted nothing"
    # B = 3 with table lengths 0, 1, tab_ld
    tables = [[], make_table(rng, V, ld, 1, bias), make_table(rng, V, ld, TAB_LD, bias)]
    if not bias:
        tables[1] = [(tables[1][0][0], 2, True, 0.0)]
    bits = make_rows(rng, 3, V, ld)
    plant_specials(bits, tables, 1, V)
    got = check(P, bits, V, 1, tables, [r] * 3, [p] * 3, [f] * 3)
    assert (got[0] == bits[0]).all() and (got[1] != bits[1]).sum() <= 1 and (got[2] != bits[2]).any()


@pytest.mark.parametrize("name", ["all_four", "repetition", "negative_p_f"])
@pytest.mark.parametrize("V,ld", SHAPES)
def test_prefix_form_row_j_sees_exactly_j_extras(P, V, ld, name):
    r, p, f, bias = PARAMS[name]
    rng = np.random.default_rng(100 * V + 50 + list(PARAMS).index(name))
    rps = 5
    for lens in ([12], [0, 1, TAB_LD]):
        B = len(lens)
        tables = [make_table(rng, V, ld, n, bias) for n in lens]
        bits = make_rows(rng, B * rps, V, ld)
        plant_specials(bits, tables, rps, V)
        extra = extras_for(rng, tables, V, ld, rps - 1)
        got = check(P, bits, V, rps, tables, [r] * B, [p] * B, [f] * B, extra=extra)
        # row 0 of a sequence sees no extra: it equals the table-only result
        alone = R.penalize_rows(bits, V, rps, tables, [r] * B, [p] * B, [f] * B)
        for b in range(B):
            assert (got[b * rps] == alone[b * rps]).all()
        assert (got != alone).any(), "the extras changed nothing"
    # a wider input row than rows_per_seq: row j still sees only 1..j
    tables = [make_table(rng, V, ld, 6, bias)]
    bits = make_rows(rng, 3, V, ld)
    check(P, bits, V, 3, tables, [r], [p], [f], extra=extras_for(rng, tables, V, ld, 6))


@pytest.mark.parametrize("V,ld", SHAPES)
def test_extras_only_rows_with_a_null_table(P, V, ld):
    rng = np.random.default_rng(V)
    bits = make_rows(rng, 8, V, ld)
    extra = [[5, 7, 7, 9], [5, V - 1, -1, V - 1]]
    got = check(P, bits, V, 4, None, [1.5, 1.0], [0.25, 2.0], [0.5, 0.0], extra=extra)
    assert (got[0] == bits[0]).all() and (got[4] == bits[4]).all()
    assert (got[2] != bits[2]).sum() == 1 and (got[3] != bits[3]).sum() == 2          # two 7s are one entry; then 7 and 9
    assert (got[7] != bits[7]).sum() == 1          # V - 1 twice, -1 ignored
    # no table and no extras: nothing to do, and allowed
    assert (run(P, bits, V, 4, None, [1.5, 1.0], [0.25, 2.0], [0.5, 0.0]) == bits).all()


@pytest.mark.parametrize("V,ld", SHAPES)
def test_chain_form_follows_the_device_counter_between_graph_replays(P, V, ld):
    from ssd_amd.utils.graphs import capture
    rng = np.random.default_rng(V + 1)
    K, B = 4, 3
    tables = [make_table(rng, V, ld, n, True) for n in (0, 1, TAB_LD)]
    bits = make_rows(rng, B, V, ld)
    plant_specials(bits, tables, 1, V)
    extra = extras_for(rng, tables, V, ld, K)
    rep, pres, freq = [1.25, 1.1, 0.8], [0.5, 0.0, -0.5], [0.0, 0.4, 0.2]
    tabs = device_tables(P, tables, TAB_LD)
    ex = torch.tensor(extra, dtype=torch.int64, device="cuda")
    step = torch.zeros(1, dtype=torch.int32, device="cuda")
    static = to_dev(bits)
    prm = (f32(rep), f32(pres), f32(freq))
    graph, stream = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with capture(graph, stream=stream):
        P.penalize_rows(static, ld, B, V, 1, *tabs[:3], TAB_LD, tabs[3], *prm, extra=ex, extra_ld=K + 1, extra_n=step)
    seen = []
    for n in (0, 1, K, 2, K + 3, -2):          # one capture; past K the counter is clamped, below 0 it is 0
        static.copy_(to_dev(bits))
        step.fill_(n)
        graph.replay()
        torch.cuda.synchronize()
        got = to_bits(static)
        want = R.penalize_rows(bits, V, 1, tables, rep, pres, freq, extra, n)
        assert (got == want).all(), n
        assert (got[:, V:] == SENTINEL).all()
        seen.append(got.copy())
        # the eager launch with the same counter gives the same bits
        assert (run(P, bits, V, 1, tables, rep, pres, freq, extra, n) == got).all()
    assert not (seen[0] == seen[1]).all() and not (seen[1] == seen[2]).all()
    assert (seen[4] == seen[2]).all() and (seen[5] == seen[0]).all()


@pytest.mark.parametrize("V,ld", SHAPES)
def test_a_sequence_with_everything_off_between_two_penalised_ones_is_untouched(P, V, ld):
    rng = np.random.default_rng(V + 2)
    rps = 5
    tables = [make_table(rng, V, ld, 10, True), [], make_table(rng, V, ld, 10, False)]
    bits = make_rows(rng, 3 * rps, V, ld)
    plant_specials(bits, tables, rps, V)
    bits[rps:2 * rps, :len(SPECIAL)] = SPECIAL
    extra = extras_for(rng, tables, V, ld, rps - 1)
    extra[1] = [0, 1, 2, 3, 4]          # the off sequence's own inputs sit on its special values
    got = check(P, bits, V, rps, tables, [1.3, 1.0, 1.0], [0.5, 0.0, 0.0], [0.1, 0.0, 0.7], extra=extra)
    assert (got[rps:2 * rps] == bits[rps:2 * rps]).all()
    assert (got[:rps] != bits[:rps]).any() and (got[2 * rps:] != bits[2 * rps:]).any()
    # off, but with a history table (a request whose penalties are all default keeps none; a table alone must still change nothing)
    tables[1] = [(t, 2, True, 0.0) for t in range(len(SPECIAL))]
    got = check(P, bits, V, rps, tables, [1.3, 1.0, 1.0], [0.5, 0.0, 0.0], [0.1, 0.0, 0.7], extra=extra)
    assert (got[rps:2 * rps] == bits[rps:2 * rps]).all()


def test_two_runs_of_the_same_input_are_bit_identical(P):
    V, ld = SHAPES[1]
    rng = np.random.default_rng(11)
    rps = 5
    tables = [make_table(rng, V, ld, n, True) for n in (7, TAB_LD, 1)]
    bits = make_rows(rng, 3 * rps, V, ld)
    plant_specials(bits, tables, rps, V)
    extra = extras_for(rng, tables, V, ld, rps - 1)
    args = (bits, V, rps, tables, [1.2, 0.9, 1.0], [0.5, -0.5, 0.0], [0.25, 0.0, 1.0])
    a = check(P, *args, extra=extra)
    b = run(P, *args, extra=extra)
    assert (a == b).all()


def test_each_refusal_code(P):
    import ctypes as C
    lib = P.load_penalty_library()
    x = torch.zeros(2, 16, dtype=torch.bfloat16, device="cuda")
    i = torch.zeros(2, 4, dtype=torch.int32, device="cuda")
    fl = torch.zeros(2, 4, dtype=torch.float32, device="cuda")
    ex = torch.zeros(2, 4, dtype=torch.int64, device="cuda")
    n = torch.zeros(2, dtype=torch.int32, device="cuda")
    one = torch.ones(2, dtype=torch.float32, device="cuda")
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    good = dict(logits=x, ld=16, T=2, V=16, rps=1, ids=i, cnt=i, bias=fl, tab_ld=4, len=n, rep=one, pres=one, freq=one, extra=None,
                extra_ld=0, extra_n=None)

    def call(**kw):
        a = dict(good, **kw)
        return lib.ssd_penalize_rows(p(a["logits"]), a["ld"], a["T"], a["V"], a["rps"], p(a["ids"]), p(a["cnt"]), p(a["bias"]), a["tab_ld"],
                                     p(a["len"]), p(a["rep"]), p(a["pres"]), p(a["freq"]), p(a["extra"]), a["extra_ld"], p(a["extra_n"]),
                                     None)
    SHAPE, ARG = -1, -3          # SSD_ERR_SHAPE, SSD_ERR_ARG (include/ssd_hip.h)
    for kw in (dict(T=0), dict(T=-1), dict(V=0), dict(rps=0), dict(ld=8), dict(tab_ld=0), dict(extra=ex, extra_ld=0),
               dict(extra=ex, extra_ld=P.MAX_EXTRA + 2, extra_n=n), dict(extra=ex, extra_ld=4, rps=5)):
        assert call(**kw) == SHAPE, kw
    for kw in (dict(logits=None), dict(rep=None), dict(pres=None), dict(freq=None), dict(len=None), dict(ids=None), dict(cnt=None),
               dict(bias=None), dict(extra_n=n)):
        assert call(**kw) == ARG, kw
    assert call() == 0 and call(ids=None, cnt=None, bias=None, len=None) == 0          # a null table is "no history"
    assert call(extra=ex, extra_ld=4, rps=2) == 0 and call(extra=ex, extra_ld=4, extra_n=n) == 0
    torch.cuda.synchronize()
    from ssd_amd.hip.lib import SsdHipError
    with pytest.raises(SsdHipError, match="ssd_penalize_rows"):
        P.penalize_rows(x, 8, 2, 16, 1, i, i, fl, 4, n, one, one, one)

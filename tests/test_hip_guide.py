"""ssd_guide_walk and ssd_guide_rows (csrc/guide.hip, include/ssd_hip_guide.h) on the GPU against tests/guide_ref.py: the walk is compared
exactly, the rows by BITS over the whole [T][ld] buffer, pad columns (a NaN sentinel) included.

Shapes: V = 1000 / ld = 1024 (one slice), V = 4136 / ld = 4160 (two slices, the second 40 entries wide), V = 1003 / ld = 1011 (rows that
are not 16-byte aligned, a last chunk cut by V), and one case at V = 128256 with two rows.  Layouts: T = 1; T = 5 with rows_per_seq = 5
(prefix form: row j sees exactly j extras); the chain form with *extra_n in {0, 3, extra_ld - 1}; B = 3 with an unguided sequence
between two guided ones.  The automaton of every small case holds: a state without edges and without a default (the whole row is
banned), a default with exceptions (to -1 and to other states), states of exactly 1, 64, 65 and 4097 edges, edges on the tokens 0,
4095, 4096, V - 1 and on V and ld - 1 (which allow nothing), next states equal to n_states (they read as -1); the large case adds a
state of 70000 edges, which needs both narrowing rounds of the search.  Walks die midway (the rows behind keep their bits) and meet a negative
extra.  +-0, +-inf and two NaNs are planted at banned and at kept entries; the unused parts of every table hold poison.  Every case runs
eagerly and as a captured graph that is replayed, without recapture, with another state0 and other extras."""
import numpy as np
import pytest
import torch

from tests import guide_ref as R

pytestmark = pytest.mark.gpu

SHAPES = [(1000, 1024), (4136, 4160), (1003, 1011)]
SENTINEL = 0x7FC5
SPECIAL = [0x0000, 0x8000, 0x7F80, 0xFF80, 0x7FC1, 0xFFC0]          # +0 -0 +inf -inf NaN NaN
# the states of automaton(): what each one is there for
S_OPEN, S_DEAD, S_ONE, S_64, S_65, S_4097, S_EDGE, S_OPEN2, N_SMALL = 0, 1, 2, 3, 4, 5, 6, 7, 8


@pytest.fixture(scope="module")
def G():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ssd_amd.hip import guide_ops
    guide_ops.load_guide_library()
    return guide_ops


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


def automaton(rng, V, ld, big: int = 0):
    """The tables (guide_ref format) of one automaton with every kind of state the header speaks of.  Next states are drawn from all
    states, -1 and n (which reads as -1), so a walk can go anywhere; `big` adds a state with that many edges."""
    n = N_SMALL + (1 if big else 0)

    def nexts(m, p_ban=0.2):
        x = rng.integers(0, n, size=m)
        x[rng.random(m) < p_ban] = -1
        x[rng.random(m) < 0.1] = n          # outside [-1, n): reads as -1
        return [int(v) for v in x]

    def on(tokens, **kw):
        tokens = sorted(set(int(t) for t in tokens))
        return list(zip(tokens, nexts(len(tokens), **kw)))
    span = max(V, 4200)          # 4097 distinct tokens need more than the small vocabularies hold: the ones at and past V allow nothing
    states = {
        S_OPEN: on(list(rng.choice(V, size=40, replace=False)) + [0, 4095 % V, V - 1, V, ld - 1], p_ban=0.5),
        S_ONE: [(int(rng.integers(0, V)), S_64)],
        S_64: on(rng.choice(V, size=64, replace=False), p_ban=0.0),
        S_65: on(rng.choice(V, size=65, replace=False)),
        S_4097: on(rng.choice(span, size=4097, replace=False)),
        S_EDGE: on({0, 4095, 4096, V - 1, V, ld - 1}, p_ban=0.0),
        S_OPEN2: on(list(rng.choice(V, size=300, replace=False)) + [V - 1], p_ban=0.9),
    }
    if big:
        states[N_SMALL] = on(rng.choice(V, size=big, replace=False))
    states[S_EDGE] = [(t, S_OPEN) for t, _ in states[S_EDGE]]                     # all valid: what is below V is allowed, the rest is not
    a = R.tables_from(n, states, {S_OPEN: S_OPEN2, S_OPEN2: n - 1})
    assert len(states[S_64]) == 64 and len(states[S_65]) == 65 and len(states[S_4097]) == 4097 and not states.get(S_DEAD)
    return a


class Tables:
    """Device tables for B slots at small strides; what a slot does not use holds poison (offsets, defaults and edges that would allow
    and ban entries if they were read), and so does the whole slot of an unguided sequence."""

    def __init__(self, autos, pad_states: int = 3, pad_edges: int = 5):
        B = len(autos)
        self.states_ld = max([a["n"] for a in autos if a is not None] + [2]) + pad_states
        self.edges_ld = max([len(a["tok"]) for a in autos if a is not None] + [8]) + pad_edges
        self.h = dict(n=np.full(B, 2, np.int32), off=np.full((B, self.states_ld + 1), 3, np.int32), dflt=np.full((B, self.states_ld), -1, np.int32),
                      tok=np.full((B, self.edges_ld), 5, np.int32), next=np.zeros((B, self.edges_ld), np.int32))
        self.h["off"][:, 0] = 0
        self.fill(autos)
        self.d = {k: i32(v) for k, v in self.h.items()}

    def fill(self, autos):
        for b, a in enumerate(autos):
            if a is None:
                continue
            h = self.h
            h["n"][b] = a["n"]
            h["off"][b, :len(a["off"])] = a["off"]
            h["dflt"][b, :a["n"]] = a["dflt"][:a["n"]]
            h["tok"][b, :len(a["tok"])] = a["tok"]
            h["next"][b, :len(a["next"])] = a["next"]

    def update(self, autos):
        self.fill(autos)
        for k, v in self.h.items():
            self.d[k].copy_(i32(v))

    @property
    def args(self):
        d = self.d
        return (d["n"], d["off"], d["dflt"], d["tok"], d["next"], self.states_ld, self.edges_ld)


def pipeline(G, tabs, d_rows, ld, T, V, rps, d_state, d_on, d_state0, d_extra=None, extra_ld=0, d_extra_n=None):
    G.guide_walk(d_state, T, rps, d_on, d_state0, *tabs.args, extra=d_extra, extra_ld=extra_ld, extra_n=d_extra_n)
    G.guide_rows(d_rows, ld, T, V, d_state, rps, *tabs.args)


def reference(bits, V, rps, autos, on, state0, extra, extra_n, edges_ld):
    T = bits.shape[0]
    st = R.walk(T, rps, autos, on, state0, extra, extra_n, edges_ld)
    return st, R.guide_rows(bits, V, rps, autos, st, edges_ld)


def plant_specials(rng, bits, V, rps, autos, on, state0, extra=None, extra_n=None):
    """SPECIAL at six banned and six kept entries of every row that has both (found with the reference: it only decides where)."""
    _, probe = reference(np.zeros_like(bits), V, rps, autos, on, state0, extra, extra_n, None)
    for r in range(bits.shape[0]):
        ban = np.nonzero(probe[r, :V] == R.NINF)[0]
        keep = np.nonzero(probe[r, :V] != R.NINF)[0]
        for pool in (ban, keep):
            if len(pool):
                for v, t in zip(SPECIAL, rng.permutation(pool)[:len(SPECIAL)]):
                    bits[r, t] = v


def check(G, bits, V, rps, autos, on, state0, extra=None, extra_n=None, second=None):
    """One case eagerly and as a captured graph.  second = (on, state0, extra, extra_n-or-None): the data the same graph is replayed
    with, without recapture.  Returns (states, bits) of the eager run."""
    from ssd_amd.utils.graphs import capture
    T, ld = bits.shape
    tabs = Tables(autos)
    E = len(extra[0]) if extra is not None else 0
    d_on, d_s0 = i32(on), i32(state0)
    d_ex = torch.tensor(extra, dtype=torch.int64, device="cuda") if extra is not None else None
    d_n = torch.tensor([extra_n], dtype=torch.int32, device="cuda") if extra_n is not None else None
    want_st, want = reference(bits, V, rps, autos, on, state0, extra, extra_n, tabs.edges_ld)

    def compare(got_st, got, want_st, want, src, what):
        assert got_st.tolist() == want_st.tolist(), what
        bad = np.argwhere(got != want)
        assert bad.size == 0, (what, [(int(r), int(c), hex(src[r, c]), hex(got[r, c]), hex(want[r, c])) for r, c in bad[:8]])
        assert (got[:, V:] == SENTINEL).all(), what
        assert (got[got != src] == R.NINF).all(), what          # only -inf is ever written

    d_state = torch.full((T + 3,), 77, dtype=torch.int32, device="cuda")          # (three entries behind the rows: never written)
    d = to_dev(bits)
    pipeline(G, tabs, d, ld, T, V, rps, d_state, d_on, d_s0, d_ex, E, d_n)
    torch.cuda.synchronize()
    st, got = d_state.cpu().numpy(), to_bits(d)
    assert st[T:].tolist() == [77] * 3
    compare(st[:T], got, want_st, want, bits, "eager")
    # the same launches captured once
    static = to_dev(bits)
    d_state.fill_(77)
    graph, stream = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with capture(graph, stream=stream):
        pipeline(G, tabs, static, ld, T, V, rps, d_state, d_on, d_s0, d_ex, E, d_n)
    static.copy_(to_dev(bits))
    graph.replay()
    torch.cuda.synchronize()
    compare(d_state.cpu().numpy()[:T], to_bits(static), want_st, want, bits, "graph")
    if second is not None:
        on2, state02, extra2, n2 = second
        d_on.copy_(i32(on2))
        d_s0.copy_(i32(state02))
        if extra is not None:
            d_ex.copy_(torch.tensor(extra2, dtype=torch.int64))
        if extra_n is not None:
            d_n.fill_(n2)
        static.copy_(to_dev(bits))
        graph.replay()
        torch.cuda.synchronize()
        w_st, w = reference(bits, V, rps, autos, on2, state02, extra2 if extra is not None else None, n2 if extra_n is not None else None,
                            tabs.edges_ld)
        compare(d_state.cpu().numpy()[:T], to_bits(static), w_st, w, bits, "graph, replayed with other data")
    return st[:T], got


def eager_then_graph(launch, read, reset, change):
    """launch() enqueues kernels over static device buffers, reset() restores what they overwrite, read() copies the outputs to the
    host, change() rewrites inputs in device memory.  Runs eagerly, then captured once and replayed (which must give the eager
    result), then replayed again, without recapture, behind change().  Returns (eager result, result with the changed inputs)."""
    from ssd_amd.utils.graphs import capture
    reset()
    launch()
    torch.cuda.synchronize()
    eager = read()
    graph, stream = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    reset()
    torch.cuda.synchronize()
    with capture(graph, stream=stream):
        launch()
    reset()
    graph.replay()
    torch.cuda.synchronize()
    again = read()
    assert all((x == y).all() for x, y in zip(eager, again)), "the captured graph differs from the eager launch"
    change()
    reset()
    graph.replay()
    torch.cuda.synchronize()
    return eager, read()


def path(rng, a, V, s, m, die_at=None, negative_at=None):
    """m tokens that lead from state s through allowed tokens (while the state has any), with a banned token at step die_at and a
    negative one at negative_at."""
    out = []
    for k in range(m):
        ok = R.allowed_set(a, s, V) if 0 <= s < a["n"] else np.zeros(V, bool)
        if k == negative_at:
            t = -int(rng.integers(1, 9))
        elif k == die_at and not ok.all():
            t = int(rng.choice(np.nonzero(~ok)[0]))
        elif ok.any():
            o0, o1 = R.edge_range(a, s)
            edge = [int(x) for x in a["tok"][o0:o1] if 0 <= x < V and ok[int(x)]]
            t = int(rng.choice(edge)) if edge and rng.random() < 0.8 else int(rng.choice(np.nonzero(ok)[0]))
        else:
            t = int(rng.integers(0, V))
        out.append(t)
        s = -1 if t < 0 else R.delta(a, s, t)
    return out


@pytest.mark.parametrize("V,ld", SHAPES)
def test_every_kind_of_state_on_rows_given_directly(G, V, ld):
    """ssd_guide_rows alone: one row per state, a row with state -1 and one whose state is n_states (no state: untouched)."""
    rng = np.random.default_rng(V)
    a = automaton(rng, V, ld)
    states = list(range(a["n"])) + [-1, a["n"]]
    T = len(states)
    bits = make_rows(rng, T, V, ld)
    want = R.guide_rows(bits, V, T, [a], states)
    probe = want.copy()
    for r in range(T):          # specials at banned and kept entries
        for pool in (np.nonzero(probe[r, :V] == R.NINF)[0], np.nonzero(probe[r, :V] != R.NINF)[0]):
            for v, t in zip(SPECIAL, rng.permutation(pool)[:len(SPECIAL)]):
                bits[r, t] = v
    tabs = Tables([a])
    want = R.guide_rows(bits, V, T, [a], states, tabs.edges_ld)
    d, d_states, src = to_dev(bits), i32(states), to_dev(bits)
    rolled = states[1:] + states[:1]          # the replay: every row at its neighbour's state
    (got,), (got2,) = eager_then_graph(lambda: G.guide_rows(d, ld, T, V, d_states, T, *tabs.args), lambda: (to_bits(d),),
                                       lambda: d.copy_(src), lambda: d_states.copy_(i32(rolled)))
    assert (got2 == R.guide_rows(bits, V, T, [a], rolled, tabs.edges_ld)).all() and (got2[:, V:] == SENTINEL).all()
    bad = np.argwhere(got != want)
    assert bad.size == 0, [(int(r), int(c), hex(bits[r, c]), hex(got[r, c]), hex(want[r, c])) for r, c in bad[:8]]
    assert (got[:, V:] == SENTINEL).all()
    assert (got[S_DEAD, :V] == R.NINF).all()                                    # no edges, no default: the whole row
    assert (got[-1] == bits[-1]).all() and (got[-2] == bits[-2]).all()          # -1 and "no state": untouched
    kept = lambda r: set(np.nonzero(got[r, :V] != R.NINF)[0].tolist())          # (a planted -inf at a kept entry is not among them)
    was_ninf = lambda r: set(np.nonzero(bits[r, :V] == R.NINF)[0].tolist())
    assert kept(S_ONE) == {int(a["tok"][a["off"][S_ONE]])} and 40 <= len(kept(S_64)) <= 64
    assert kept(S_EDGE) <= {0, 4095, 4096, V - 1} and {0, V - 1} <= kept(S_EDGE) | was_ninf(S_EDGE)
    o0, o1 = a["off"][S_OPEN], a["off"][S_OPEN + 1]
    banned = [int(t) for t, x in zip(a["tok"][o0:o1], a["next"][o0:o1]) if not 0 <= x < a["n"] and t < V]
    open_row = np.nonzero(got[S_OPEN] != bits[S_OPEN])[0].tolist()
    assert set(open_row) <= set(banned) and len(banned) > 3          # a default: only the exceptions to -1 (and to n_states) are written
    # twice the same input: the same bits
    d2 = to_dev(bits)
    G.guide_rows(d2, ld, T, V, i32(states), T, *tabs.args)
    torch.cuda.synchronize()
    assert (to_bits(d2) == got).all()


@pytest.mark.parametrize("V,ld", SHAPES)
def test_one_row_five_rows_and_three_sequences(G, V, ld):
    rng = np.random.default_rng(100 * V + 1)
    a = automaton(rng, V, ld)
    # T = 1, without extras: every state in turn through one captured graph would be a test of its own; here two of them
    bits = make_rows(rng, 1, V, ld)
    plant_specials(rng, bits, V, 1, [a], [1], [S_65])
    st, got = check(G, bits, V, 1, [a], [1], [S_65], second=([1], [S_4097], None, None))
    assert st.tolist() == [S_65] and (got != bits).any()
    # T = 5, rows_per_seq = 5: row j is guided by the state after j extras
    rps = 5
    for start, kw in ((S_OPEN, {}), (S_64, dict(die_at=2)), (S_4097, dict(negative_at=3)), (S_EDGE, {})):
        ex = [int(rng.integers(0, V))] + path(rng, a, V, start, rps - 1, **kw)
        ex2 = [int(rng.integers(0, V))] + path(rng, a, V, S_65, rps - 1)
        bits = make_rows(rng, rps, V, ld)
        plant_specials(rng, bits, V, rps, [a], [1], [start], [ex])
        st, got = check(G, bits, V, rps, [a], [1], [start], [ex], second=([1], [S_65], [ex2], None))
        assert st[0] == start
        if "die_at" in kw:          # the walk died midway (at the banned token at the latest): the rows behind are untouched
            dead = int(np.argmax(st < 0))
            assert 1 <= dead <= 3 and (st[dead:] == -1).all() and (got[dead:] == bits[dead:]).all() and (got[:dead] != bits[:dead]).any()
        if "negative_at" in kw:
            assert st[4] == -1 and (got[4] == bits[4]).all()
    # B = 3: no guide in the middle, its rows on special values and its slot full of poison
    autos = [a, None, automaton(rng, V, ld)]
    starts = [S_OPEN2, 1, S_65]
    extra = [[0] + path(rng, autos[0], V, starts[0], rps - 1), [int(t) for t in rng.integers(0, V, size=rps)],
             [0] + path(rng, autos[2], V, starts[2], rps - 1, die_at=3)]
    extra2 = [[0] + path(rng, autos[0], V, S_64, rps - 1), extra[1], [0] + path(rng, autos[2], V, S_4097, rps - 1)]
    bits = make_rows(rng, 3 * rps, V, ld)
    plant_specials(rng, bits, V, rps, autos, [1, 0, 1], starts, extra)
    bits[rps:2 * rps, :len(SPECIAL)] = SPECIAL
    st, got = check(G, bits, V, rps, autos, [1, 0, 1], starts, extra, second=([1, 0, 1], [S_64, 0, S_4097], extra2, None))
    assert st[rps:2 * rps].tolist() == [-1] * rps and (got[rps:2 * rps] == bits[rps:2 * rps]).all()
    assert (got[:rps] != bits[:rps]).any() and (got[2 * rps:] != bits[2 * rps:]).any()
    # a start state outside the automaton and guide_on = 0 beside a real automaton: -1, rows untouched
    st, got = check(G, bits, V, rps, autos, [0, 0, 1], [S_OPEN, 0, autos[2]["n"]], extra)
    assert st.tolist() == [-1] * (3 * rps) and (got == bits).all()


@pytest.mark.parametrize("V,ld", SHAPES)
@pytest.mark.parametrize("n", [0, 3, 16])
def test_chain_form_with_the_counter_at_zero_three_and_extra_ld_minus_one(G, V, ld, n):
    rng = np.random.default_rng(V + n)
    E = 17
    autos = [automaton(rng, V, ld), None, automaton(rng, V, ld)]
    starts = [S_OPEN, 0, S_4097]
    extra = [[0] + path(rng, autos[0], V, starts[0], E - 1), [1] * E, [0] + path(rng, autos[2], V, starts[2], E - 1, die_at=7)]
    extra2 = [[0] + path(rng, autos[0], V, S_65, E - 1, negative_at=1), [1] * E, [0] + path(rng, autos[2], V, S_64, E - 1)]
    bits = make_rows(rng, 3, V, ld)
    plant_specials(rng, bits, V, 1, autos, [1, 0, 1], starts, extra, n)
    n2 = {0: E + 4, 3: -2, 16: 2}[n]          # past E - 1 the counter is clamped, below 0 it is 0
    st, got = check(G, bits, V, 1, autos, [1, 0, 1], starts, extra, n, second=([1, 0, 1], [S_65, 0, S_64], extra2, n2))
    assert st[1] == -1 and (got[1] == bits[1]).all()
    if n == 0:
        assert st.tolist() == [S_OPEN, -1, S_4097]
    if n == 16:
        assert st[2] == -1 and (got[2] == bits[2]).all()          # died at step 7


def test_malformed_offsets_mean_no_edges(G):
    V, ld = SHAPES[0]
    rng = np.random.default_rng(77)
    # state 0: a default and edges that ban; state 1: no default and edges that allow.  Then state 1's end offset leaves the table, or
    # state 1's offsets run backwards: either way it has no edges (all banned); state 0 keeps its own
    a = R.tables_from(2, {0: [(3, -1), (9, -1)], 1: [(4, 0), (5, 0), (6, 0)]}, {0: 1})
    for off in ([0, 2, 99], [0, 2, 1], [3, 2, 5], [-1, 2, 5]):
        b = dict(a, off=np.array(off))
        bits = make_rows(rng, 2, V, ld)
        tabs = Tables([b])
        want = R.guide_rows(bits, V, 2, [b], [0, 1], tabs.edges_ld)
        d, d_states, src = to_dev(bits), i32([0, 1]), to_dev(bits)
        (got,), (got2,) = eager_then_graph(lambda: G.guide_rows(d, ld, 2, V, d_states, 2, *tabs.args), lambda: (to_bits(d),),
                                           lambda: d.copy_(src), lambda: d_states.copy_(i32([1, 0])))
        assert (got == want).all(), off
        assert (got2 == R.guide_rows(bits, V, 2, [b], [1, 0], tabs.edges_ld)).all(), off
        if off[1] == 2 and off[0] == 0:
            assert (got[1, :V] == R.NINF).all() and got[0, 3] == R.NINF and got[0, 4] == bits[0, 4]
        else:
            assert (got[0] == bits[0]).all()          # state 0 lost its exceptions: the default allows everything
        st = torch.full((2,), 9, dtype=torch.int32, device="cuda")
        two = tuple(t.repeat(2, *[1] * (t.dim() - 1)) if torch.is_tensor(t) else t for t in tabs.args)
        on, s0, ex, one = i32([1, 1]), i32([0, 1]), torch.tensor([[0, 3], [0, 5]], dtype=torch.int64, device="cuda"), i32([1])

        def other():
            s0.copy_(i32([1, 0]))
            ex.copy_(torch.tensor([[0, 5], [0, 4]], dtype=torch.int64))
        (w,), (w2,) = eager_then_graph(lambda: G.guide_walk(st, 2, 1, on, s0, *two, extra=ex, extra_ld=2, extra_n=one),
                                       lambda: (st.cpu().numpy(),), lambda: st.fill_(9), other)
        assert w.tolist() == R.walk(2, 1, [b, b], [1, 1], [0, 1], [[0, 3], [0, 5]], 1, tabs.edges_ld).tolist(), off
        assert w2.tolist() == R.walk(2, 1, [b, b], [1, 1], [1, 0], [[0, 5], [0, 4]], 1, tabs.edges_ld).tolist(), off


def test_the_llama_vocabulary_with_two_rows_and_a_state_of_70000_edges(G):
    V = ld = 128256
    BIG = N_SMALL
    rng = np.random.default_rng(5)
    a = automaton(rng, V, ld, big=70000)
    o0, o1 = int(a["off"][BIG]), int(a["off"][BIG + 1])
    assert o1 - o0 == 70000
    tok = a["tok"][o0:o1]
    a["next"][o0 + 35000] = S_OPEN                 # a way from the big state into the default state: row 1 of the first case
    # two rows, prefix form: the 70000-edge state, then the state behind one of its edges
    ex = [7, int(tok[35000])]
    bits = make_rows(rng, 2, V, ld)
    plant_specials(rng, bits, V, 2, [a], [1], [BIG], [ex])
    st, got = check(G, bits, V, 2, [a], [1], [BIG], [ex], second=([1], [S_OPEN], [[7, int(a["tok"][0])]], None))
    assert st.tolist() == [BIG, S_OPEN]
    assert 0 < (got[1] != bits[1]).sum() < 40                                   # a default: a handful of exceptions
    assert (got[0, :V] != R.NINF).sum() <= 70000 and (got[0, :V] == R.NINF).sum() >= V - 70000
    # the walk's search over the big state: first, last and inner edges, and absent tokens below, above and between them
    absent = [t for t in (0, 1, 2, V - 1, V - 2, int(tok[100]) + 1, int(tok[69000]) - 1, int(tok[4096]) + 1) if t not in set(tok.tolist())]
    probes = [int(tok[i]) for i in (0, 1, 63, 64, 65, 4095, 4096, 4097, 34999, 35000, 69998, 69999)] + absent
    want = [R.delta(a, BIG, t) for t in probes]
    assert any(w >= 0 for w in want[:12]) and all(w == -1 for w in want[12:])          # the big state has no default
    B = len(probes)
    tabs = Tables([a])
    rep = tuple(t.expand(B, *t.shape[1:]).contiguous() if torch.is_tensor(t) else t for t in tabs.args)
    st = torch.full((B,), 9, dtype=torch.int32, device="cuda")
    on, s0, one = i32([1] * B), i32([BIG] * B), i32([1])
    ex = torch.tensor([[0, t] for t in probes], dtype=torch.int64, device="cuda")
    (w,), (w2,) = eager_then_graph(lambda: G.guide_walk(st, B, 1, on, s0, *rep, extra=ex, extra_ld=2, extra_n=one), lambda: (st.cpu().numpy(),),
                                   lambda: st.fill_(9), lambda: ex.copy_(torch.tensor([[0, t] for t in probes[::-1]], dtype=torch.int64)))
    assert w.tolist() == want and w2.tolist() == want[::-1]          # the replay: the same probes in the other order


def test_each_refusal_code(G):
    import ctypes as CT
    lib = G.load_guide_library()
    x = torch.zeros(2, 16, dtype=torch.bfloat16, device="cuda")
    i = torch.zeros(2, 64, dtype=torch.int32, device="cuda")
    ex = torch.zeros(2, 4, dtype=torch.int64, device="cuda")
    n = torch.zeros(2, dtype=torch.int32, device="cuda")
    st = torch.full((2,), -1, dtype=torch.int32, device="cuda")
    p = lambda t: None if t is None else CT.c_void_p(t.data_ptr())
    good = dict(rows=x, ld=16, T=2, V=16, st=st, rps=1, on=n, s0=n, n=n, off=i, dflt=i, tok=i, nxt=i, sld=4, eld=8, extra=None, extra_ld=0,
                extra_n=None)

    def walk(**kw):
        a = dict(good, **kw)
        return lib.ssd_guide_walk(p(a["st"]), a["T"], a["rps"], p(a["on"]), p(a["s0"]), p(a["n"]), p(a["off"]), p(a["dflt"]), p(a["tok"]),
                                  p(a["nxt"]), a["sld"], a["eld"], p(a["extra"]), a["extra_ld"], p(a["extra_n"]), None)

    def rows(**kw):
        a = dict(good, **kw)
        return lib.ssd_guide_rows(p(a["rows"]), a["ld"], a["T"], a["V"], p(a["st"]), a["rps"], p(a["n"]), p(a["off"]), p(a["dflt"]),
                                  p(a["tok"]), p(a["nxt"]), a["sld"], a["eld"], None)
    SHAPE, ARG = -1, -3          # SSD_ERR_SHAPE, SSD_ERR_ARG (include/ssd_hip.h)
    for kw in (dict(T=0), dict(T=-1), dict(T=65536), dict(rps=0), dict(sld=0), dict(eld=0), dict(eld=G.MAX_EDGES + 1), dict(extra=ex, extra_ld=0),
               dict(extra=ex, extra_ld=G.MAX_EXTRA + 2, extra_n=n), dict(extra=ex, extra_ld=4, rps=5)):
        assert walk(**kw) == SHAPE, kw
    for kw in (dict(st=None), dict(on=None), dict(s0=None), dict(n=None), dict(off=None), dict(dflt=None), dict(tok=None), dict(nxt=None),
               dict(extra_n=n)):
        assert walk(**kw) == ARG, kw
    for kw in (dict(T=0), dict(T=65536), dict(V=0), dict(rps=0), dict(ld=8), dict(sld=0), dict(eld=0), dict(eld=G.MAX_EDGES + 1)):
        assert rows(**kw) == SHAPE, kw
    for kw in (dict(rows=None), dict(st=None), dict(n=None), dict(off=None), dict(dflt=None), dict(tok=None), dict(nxt=None)):
        assert rows(**kw) == ARG, kw
    assert walk() == 0 and rows() == 0 and walk(extra=ex, extra_ld=4, rps=2) == 0 and walk(extra=ex, extra_ld=4, extra_n=n) == 0
    torch.cuda.synchronize()
    assert st.tolist() == [-1, -1] and (x == 0).all()          # n_states 0: no state is one, nothing was written
    from ssd_amd.hip.lib import SsdHipError
    with pytest.raises(SsdHipError, match="ssd_guide_rows"):
        G.guide_rows(x, 8, 2, 16, st, 1, n, i, i, i, i, 4, 8)

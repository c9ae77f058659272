"""Guided decoding: a deterministic automaton over token ids whose current state yields the set of tokens that may come next
(include/ssd_hip_guide.h has the device side and the normative semantics).

``TokenAutomaton(num_states, start, edges, default=None)`` has the states ``0 .. num_states - 1``.  ``edges`` maps a state to
``{token id: next state}``; ``default`` maps a state to the next state of every token that has no edge there.  A state missing from
``default``, or the value -1, means "no such token"; -1 is also accepted as an edge's next state and bans that token explicitly (the
exception form at a state with a default).  ``delta(s, t)`` is the edge's next state if the edge (s, t) exists, otherwise
``default[s]``, otherwise -1, and ``delta(-1, t) = -1``.  Token t is allowed at state s if and only if ``delta(s, t) != -1``.

The object is immutable.  It keeps the flattened form the device tables hold -- CSR offsets ``edge_off`` [num_states + 1], ``dflt``
[num_states], and ``edge_tok`` / ``edge_next`` [num_edges] with every state's edges sorted by token -- and the host-side ``delta``.

Compilers from strings, regular expressions or JSON schemas to an automaton need a tokenizer and are not part of this package;
``from_choices`` covers the one case that needs none: the request must answer with exactly one of several token sequences."""
from __future__ import annotations

import numpy as np

MAX_STATES = 16384      # SSD_GUIDE_MAX_STATES
MAX_EDGES = 262144      # SSD_GUIDE_MAX_EDGES


def _is_int(v) -> bool:
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


class TokenAutomaton:
    __slots__ = ("num_states", "start", "num_edges", "max_token", "edge_off", "dflt", "edge_tok", "edge_next", "_edges", "_frozen")

    def __init__(self, num_states: int, start: int, edges, default=None, *, _what: str = "TokenAutomaton"):
        if not _is_int(num_states) or num_states < 1:
            raise ValueError(f"{_what}: num_states must be an integer >= 1, got {num_states!r}")
        if num_states > MAX_STATES:
            raise ValueError(f"{_what}: num_states = {num_states}: at most {MAX_STATES} states")
        if not _is_int(start) or not 0 <= start < num_states:
            raise ValueError(f"{_what}: start must be a state in [0, {num_states}), got {start!r}")
        if not isinstance(edges, dict) or not all(isinstance(v, dict) for v in edges.values()):
            raise ValueError(f"{_what}: edges must map a state to {{token id: next state}}, got {type(edges).__name__}")
        if default is not None and not isinstance(default, dict):
            raise ValueError(f"{_what}: default must map a state to a next state or be None, got {type(default).__name__}")
        n = int(num_states)
        dflt = np.full(n, -1, dtype=np.int32)
        for s, nx in (default or {}).items():
            if not _is_int(s) or not 0 <= s < n:
                raise ValueError(f"{_what}: default holds the state {s!r}, which is not in [0, {n})")
            if not _is_int(nx) or not -1 <= nx < n:
                raise ValueError(f"{_what}: default of state {s} is {nx!r}, which is neither -1 nor a state in [0, {n})")
            dflt[s] = nx
        total = 0
        for s, out in edges.items():
            if not _is_int(s) or not 0 <= s < n:
                raise ValueError(f"{_what}: edges holds the state {s!r}, which is not in [0, {n})")
            total += len(out)
        if total > MAX_EDGES:
            raise ValueError(f"{_what}: edges holds {total} edges: at most {MAX_EDGES}")
        off = np.zeros(n + 1, dtype=np.int32)
        tok = np.empty(total, dtype=np.int32)
        nxt = np.empty(total, dtype=np.int32)
        kept: dict[int, dict[int, int]] = {}
        max_token, at = -1, 0
        for s in range(n):
            out = edges.get(s)
            if out:
                m = len(out)
                t = np.fromiter(out.keys(), dtype=object, count=m)
                v = np.fromiter(out.values(), dtype=object, count=m)
                if not all(_is_int(x) for x in t) or min(t) < 0 or max(t) > 2 ** 31 - 1:
                    raise ValueError(f"{_what}: edges of state {s} hold a token id that is not an integer in [0, 2**31)")
                if not all(_is_int(x) for x in v) or min(v) < -1 or max(v) >= n:
                    raise ValueError(f"{_what}: edges of state {s} lead to a next state that is neither -1 nor a state in [0, {n})")
                t, v = t.astype(np.int64), v.astype(np.int64)
                order = np.argsort(t, kind="stable")
                tok[at:at + m], nxt[at:at + m] = t[order], v[order]
                kept[s] = {int(a): int(b) for a, b in zip(t, v)}
                max_token = max(max_token, int(t.max()))
                at += m
            off[s + 1] = at
        object.__setattr__(self, "_frozen", False)
        self.num_states, self.start, self.num_edges, self.max_token = n, int(start), total, max_token
        self.edge_off, self.dflt, self.edge_tok, self.edge_next = off, dflt, tok, nxt
        for a in (off, dflt, tok, nxt):
            a.setflags(write=False)
        self._edges = kept
        if not self.any_allowed(self.start):
            raise ValueError(f"{_what}: nothing is allowed at the start state {self.start}")
        self._frozen = True

    def __setattr__(self, name, value):
        if getattr(self, "_frozen", False):
            raise AttributeError("TokenAutomaton is immutable")
        object.__setattr__(self, name, value)

    def delta(self, s: int, t: int) -> int:
        """The state after token t at state s; -1: t is not allowed there (or s is -1 already)."""
        if not 0 <= s < self.num_states:
            return -1
        nx = self._edges.get(s, {}).get(int(t))
        return int(self.dflt[s]) if nx is None else nx

    def allowed(self, s: int, t: int) -> bool:
        return self.delta(s, t) != -1

    def any_allowed(self, s: int) -> bool:
        """Some token is allowed at state s: it has a default, or an edge that does not ban its token."""
        if not 0 <= s < self.num_states:
            return False
        return self.dflt[s] != -1 or any(nx != -1 for nx in self._edges.get(s, {}).values())

    def walk(self, s: int, tokens) -> int:
        for t in tokens:
            s = self.delta(s, t)
        return s

    def __repr__(self) -> str:
        return f"TokenAutomaton(num_states={self.num_states}, start={self.start}, num_edges={self.num_edges})"

    @classmethod
    def from_choices(cls, choices, eos: int, *, _what: str = "TokenAutomaton.from_choices") -> "TokenAutomaton":
        """The trie of `choices` (non-empty lists of token ids; shared prefixes are merged): at the end of every choice the only way on
        is `eos`, which leads to a state where nothing is allowed.  One choice may be a prefix of another: there `eos` and the
        continuation are both allowed.  A choice cannot contain `eos` itself."""
        if not _is_int(eos) or eos < 0:
            raise ValueError(f"{_what}: eos must be an integer >= 0, got {eos!r}")
        edges, ends = check_choices(choices, _what)
        for c in choices:
            if eos in c:
                raise ValueError(f"{_what}: the choice {list(c)!r} holds the EOS {eos}, which would end it early")
        final = len(edges)          # behind the EOS: no edges, no default
        for s in ends:
            edges[s][int(eos)] = final
        return cls(final + 1, 0, edges, None, _what=_what)


def check_choices(choices, what: str = "TokenAutomaton.from_choices", trie: bool = True):
    """The trie of `choices` without the EOS -- (edges, the state each choice ends at) -- after the checks that do not need the EOS: the
    shape, and the limits of the automaton from_choices will build (the EOS adds one state, and one edge per distinct choice, whatever
    its id).  SamplingParams checks guided_choice_ids with it; the automaton itself is built where the EOS is known, so with
    trie=False the trie is only built where it is needed to decide -- a trie has at most one state per token, so a list whose
    tokens + 2 fit the state limit fits both limits -- and None is returned otherwise."""
    if (not isinstance(choices, (list, tuple)) or not choices
            or not all(isinstance(c, (list, tuple)) and len(c) > 0 and all(_is_int(t) and t >= 0 for t in c) for c in choices)):
        raise ValueError(f"{what}: choices must be a non-empty list of non-empty lists of integers >= 0, got {choices!r}")
    if not trie and sum(len(c) for c in choices) + 2 <= MAX_STATES:         # (edges <= tokens + choices <= 2 * tokens < MAX_EDGES)
        return None
    edges: dict[int, dict[int, int]] = {0: {}}
    ends = []
    for c in choices:
        s = 0
        for t in c:
            nx = edges[s].get(int(t))
            if nx is None:
                nx = edges[s][int(t)] = len(edges)
                edges[nx] = {}
            s = nx
        ends.append(s)
    n, m = len(edges) + 1, sum(len(out) for out in edges.values()) + len(set(ends))
    if n > MAX_STATES:
        raise ValueError(f"{what}: the choices need {n} states: at most {MAX_STATES}")
    if m > MAX_EDGES:
        raise ValueError(f"{what}: the choices need {m} edges: at most {MAX_EDGES}")
    return edges, ends

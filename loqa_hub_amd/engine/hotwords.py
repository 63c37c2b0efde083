"""Hotword phrases compiled into an Aho-Corasick automaton (host side).

``compile_hotwords`` tokenizes every phrase twice with the engine's tokenizer
(``" " + p``: how Whisper spells a word in mid-sentence; ``p``: at the start),
builds the trie of the token sequences, numbers its nodes breadth-first (root
0) and computes the failure links. ``HotwordAutomaton`` keeps the trie for the
chain-walking reference (``ops.reference.hotword_advance`` / ``hotword_boosted``
/ ``hotword_step``) and the flattened table the device reads
(csrc/kernels/hotword.hip), and finds the phrases a transcript contains.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np

from ..config import _hotword_list
from ..ops.reference import (HOTWORD_MAX_PHRASES, HOTWORD_MAX_TOKENS, HOTWORD_N_CAP,
                             HOTWORD_T_CAP)


def normalize_phrases(phrases) -> list[str]:
    """Stripped, inner whitespace collapsed, empty ones dropped, duplicates
    collapsed (first occurrence kept)."""
    if phrases is None:
        return []
    if isinstance(phrases, str):
        raise ValueError("hotwords: a list of phrases, not one string")
    return _hotword_list(phrases)


def check_boost(boost) -> float:
    try:
        b = float(boost)
    except (TypeError, ValueError):
        raise ValueError(f"hotword boost {boost!r}: a finite number") from None
    if not math.isfinite(b) or abs(b) > float(np.finfo(np.float32).max):
        raise ValueError(f"hotword boost {boost!r}: a finite f32 number")
    return b


@dataclass
class HotwordAutomaton:
    phrases: list                     # normalised phrases, in input order
    boost: float                      # logit units, added once per eligible column
    sequences: list                   # distinct (tokens tuple), in trie insertion order
    edges: list                       # per node {token: child}
    fail: list                        # per node its failure link (root: 0)
    terminal: list                    # per node the phrase indices whose sequence ends there
    off: np.ndarray = field(default=None, repr=False)    # int32 [N + 1]
    tok: np.ndarray = field(default=None, repr=False)    # int32 [T]
    dst: np.ndarray = field(default=None, repr=False)    # int32 [T]

    @property
    def N(self) -> int:
        return len(self.edges)

    @property
    def T(self) -> int:
        return int(self.off[-1])

    def chain(self, n: int) -> list:
        """``n, fail[n], ..., 0``."""
        out = [n]
        while n:
            n = self.fail[n]
            out.append(n)
        return out

    def header(self) -> np.ndarray:
        """int32 [4]: N, T, the bits of the f32 boost, 0."""
        h = np.zeros(4, np.int32)
        h[0], h[1] = self.N, self.T
        h[2] = np.float32(self.boost).view(np.int32)
        return h

    def span(self, n: int) -> tuple[np.ndarray, np.ndarray]:
        a, b = int(self.off[n]), int(self.off[n + 1])
        return self.tok[a:b], self.dst[a:b]

    def advance_flat(self, n: int, t: int) -> int:
        """``advance`` on the flattened table, as the device does it: ``t`` in
        span(n), else in span(0), else the root."""
        for m in ((n, 0) if n else (0,)):
            tk, ds = self.span(m)
            i = int(np.searchsorted(tk, t))
            if i < len(tk) and int(tk[i]) == t:
                return int(ds[i])
        return 0

    def boosted_flat(self, n: int) -> set:
        out = set(int(x) for x in self.span(0)[0])
        if n:
            out |= set(int(x) for x in self.span(n)[0])
        return out

    def matches(self, tokens) -> list:
        """Indices into ``phrases`` of the phrases one of whose token sequences
        occurs in ``tokens``, in the order their first occurrence ends."""
        from ..ops.reference import hotword_advance
        out, n = [], 0
        for t in tokens:
            n = hotword_advance(self, n, int(t))
            for m in self.chain(n):
                for p in self.terminal[m]:
                    if p not in out:
                        out.append(p)
        return out


def compile_hotwords(phrases, boost: float, encode, vocab_size: int) -> HotwordAutomaton:
    """The automaton of ``phrases`` under ``encode`` (text -> token ids).
    ``ValueError`` (naming the phrase) for more than ``HOTWORD_MAX_PHRASES``
    phrases, a variant of more than ``HOTWORD_MAX_TOKENS`` tokens, a token id at
    or above ``vocab_size``, and when the flattened table exceeds its capacity."""
    boost = check_boost(boost)
    phrases = normalize_phrases(phrases)
    if len(phrases) > HOTWORD_MAX_PHRASES:
        raise ValueError(f"hotwords: {len(phrases)} phrases exceed the limit of "
                         f"{HOTWORD_MAX_PHRASES} (first beyond it: {phrases[HOTWORD_MAX_PHRASES]!r})")
    # the trie, in insertion order; sequences[i] ends at node ends[i]
    kids: list[dict] = [{}]
    term: list[list] = [[]]
    sequences: list = []
    for pi, p in enumerate(phrases):
        for text in (" " + p, p):
            seq = tuple(int(t) for t in encode(text))
            if not seq:
                continue
            if len(seq) > HOTWORD_MAX_TOKENS:
                raise ValueError(f"hotword {p!r}: {len(seq)} tokens exceed the limit of "
                                 f"{HOTWORD_MAX_TOKENS} per variant")
            bad = [t for t in seq if not 0 <= t < vocab_size]
            if bad:
                raise ValueError(f"hotword {p!r}: token id {bad[0]} is outside the vocabulary "
                                 f"of {vocab_size}")
            n = 0
            for t in seq:
                if t not in kids[n]:
                    kids[n][t] = len(kids)
                    kids.append({})
                    term.append([])
                n = kids[n][t]
            if not term[n]:             # a sequence seen before ends at the same node
                sequences.append(seq)
            if pi not in term[n]:
                term[n].append(pi)
    # breadth-first numbering, a node's children in ascending token order
    order, new_id = [0], {0: 0}
    for old in order:
        for t in sorted(kids[old]):
            c = kids[old][t]
            new_id[c] = len(order)
            order.append(c)
    N = len(order)
    assert N <= HOTWORD_N_CAP
    edges = [{t: new_id[c] for t, c in sorted(kids[old].items())} for old in order]
    terminal = [tuple(term[old]) for old in order]
    # failure links, in BFS order (a parent's link is known before its children's)
    fail = [0] * N
    for n in range(1, N):               # the root's children keep 0
        for t, c in edges[n].items():
            f = fail[n]
            while f and t not in edges[f]:
                f = fail[f]
            fail[c] = edges[f].get(t, 0)
    auto = HotwordAutomaton(phrases, boost, sequences, edges, fail, terminal)
    # the flattened table: span 0 = the root's edges, span n > 0 = the union of
    # the edges of the non-root nodes of chain(n), the deepest node's target
    off = np.zeros(N + 1, np.int64)
    toks, dsts = [], []
    for n in range(N):
        if n == 0:
            merged = dict(edges[0])
        else:
            merged = {}
            for m in auto.chain(n)[:-1]:
                for t, c in edges[m].items():
                    merged.setdefault(t, c)
        for t in sorted(merged):
            toks.append(t)
            dsts.append(merged[t])
        off[n + 1] = len(toks)
        if len(toks) > HOTWORD_T_CAP:
            raise ValueError(f"hotwords: the flattened automaton exceeds {HOTWORD_T_CAP} table "
                             f"entries (at node {n} of {N}); use fewer or shorter phrases")
    auto.off = off.astype(np.int32)
    auto.tok = np.asarray(toks, np.int32)
    auto.dst = np.asarray(dsts, np.int32)
    return auto

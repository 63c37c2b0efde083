"""Beam search decoding for the STT engine (``STTEngine(beam_size=B)``):
openai/whisper's ``BeamSearchDecoder`` + ``MaximumLikelihoodRanker`` with
patience 1 and no length penalty, per 30 s window.

A window's prompt (the SOT probe step included) is fed through one decoder
sequence as in the greedy engine. The step that feeds its last prompt token is
the search's first: ``ops.beam_topk`` on that one row, ``ops.beam_merge`` with
``n_src = 1``. From then on the window is a *group* of B rows that own B pool
sequences of equal length; ``phys[i]`` is the sequence beam i reads and
appends to. After a step the host reads the merge results and re-parents: the
first child of a parent inherits its sequence, every further child takes a
sequence that no beam inherits and gets the parent's used blocks - all such
copies of a step, of every group, in one ``ops.kv_copy_blocks`` launch (the
first step forks the prompt this way). The beams of a group share the window's
cross-attention slot.

One synchronous step at a time: the eager fast / fused forward
(``STTEngine._step`` without graphs), the row scans, a read-back. Groups batch
with each other, with windows still in their prompt and with teacher-forced
requests (one row, no beams) under the engine's token budget.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import ops
from ..ops.reference import BeamState


class _Row:
    """One decoder row of a step, as ``STTEngine._host_meta`` reads a request."""
    __slots__ = ("seq_id", "slot", "feed", "sot_pending")

    def __init__(self, seq_id: int, slot: int, feed: list, sot_pending: bool = False):
        self.seq_id, self.slot, self.feed, self.sot_pending = seq_id, slot, feed, sot_pending


class BeamGroup:
    """A window being searched: the host state of the search and the pool
    sequences of its beams."""

    def __init__(self, B: int, eot: int, max_new: int, seq_id: int):
        self.state = BeamState(B, eot, max_new)
        self.seqs = [seq_id]        # every pool sequence the group owns
        self.phys = [seq_id]        # beam i -> its sequence


class BeamDecoder:
    def __init__(self, engine):
        self.e = engine
        self.B = engine.beam_size
        self.logits = None          # the last step's logits (STTEngine._sample leaves them here)
        self._rr = 0
        dev = engine.device
        self._rows0 = torch.zeros(128, dtype=torch.int32, device=dev)

    # ------------------------------------------------------------ one step
    def decode_once(self, live: list) -> list:
        e, B = self.e, self.B
        n = len(live)
        order = [live[(self._rr + i) % n] for i in range(n)]
        self._rr = (self._rr + 1) % n
        left = e.step_tokens
        plain, first, groups = [], [], []     # (request, fed tokens, rest of its feed)
        for r in order:
            if r.beam is not None:
                if B <= left:
                    groups.append(r)
                    left -= B
                continue
            k = min(len(r.feed), len(e.sot), left)
            if k <= 0:
                continue
            left -= k
            item = (r, r.feed[:k], r.feed[k:])
            searching = r.target is None and not item[2] and not r.sot_pending
            (first if searching else plain).append(item)
        # rows: the plain ones, the windows at their first search step, the groups
        rows, sot = [], []
        for r, feed, rest in plain + first:
            rows.append(_Row(r.seq_id, r.slot, feed))
            sot.append(bool(r.sot_pending and not rest))
        for r in groups:
            for i, (toks, _) in enumerate(r.beam.state.beams):
                rows.append(_Row(r.beam.phys[i], r.slot, [toks[-1]]))
                sot.append(False)
        if not rows:
            return []
        self.logits = None
        res = e._step(rows, sot if e.sot_probe else None)
        nxt, lps, plps = res if e.row_fields else (res[0], res[1], None)
        e.stats["decode_steps"] += 1
        done = []
        for j, (r, feed, rest) in enumerate(plain):
            if rest:                       # part of the prompt still to feed: logits unused
                r.feed = rest
            elif r.sot_pending:            # the SOT step: language and no_speech_prob
                r.feed = e._sot_result(r, int(nxt[j]), float(lps[j]), float(plps[j]))
            else:                          # teacher-forced: one row, no beams
                t = int(r.target[r.step])
                r.tokens.append(t)
                r.step += 1
                if t == e.eot or len(r.tokens) >= r.max_new_tokens or r.step >= len(r.target):
                    f = e._finish(r)
                    if f is not None:
                        done.append(f)
                else:
                    r.feed = [t]
        if first or groups:
            done += self._search(len(plain), [r for r, _, _ in first], groups)
        return done

    # ----------------------------------------------------- selection + KV
    def _search(self, row0: int, first: list, groups: list) -> list:
        e, B = self.e, self.B
        for r in first:
            r.beam = BeamGroup(B, e.eot, r.max_new_tokens, r.seq_id)
            r.feed = []
            e.stats["beam_windows"] += 1
        n_rows = len(first) + B * len(groups)
        logits = self.logits[row0:row0 + n_rows]
        mask = mask_rows = None
        if e._sup is not None:             # row 0 of the table: the suppress mask
            mask, mask_rows = e._sup, self._rows0[:n_rows]
        cid, clp, elp = ops.beam_topk(logits, mask, mask_rows, e.eot, B)
        outs = []
        for reqs, n_src, lo in ((first, 1, 0), (groups, B, len(first))):
            if not reqs:
                continue
            hi = lo + len(reqs) * n_src
            cum = torch.from_numpy(np.stack([r.beam.state.cum for r in reqs])).to(e.device)
            m = ops.beam_merge(cid[lo:hi], clp[lo:hi], elp[lo:hi], cum, n_src)
            outs.append((reqs, n_src, lo, [x.cpu().numpy() for x in m]))
        cid_h, clp_h, elp_h = cid.cpu().numpy(), clp.cpu().numpy(), elp.cpu().numpy()
        done, pairs = [], []
        for reqs, n_src, lo, m in outs:
            for g, r in enumerate(reqs):
                a, b = lo + g * n_src, lo + (g + 1) * n_src
                tok, parent, lp, cum_out, eot_score, eot_fin = (x[g].copy() for x in m)
                st = r.beam.state
                if e.beam_debug is not None:
                    e.beam_debug.append({"request": r, "window": r.win, "step": st.steps,
                                         "cand_id": cid_h[a:b].copy(), "cand_lp": clp_h[a:b].copy(),
                                         "eot_lp": elp_h[a:b].copy()})
                if r.beam_force is not None:
                    # debug replay: beam i follows the given tokens in row i
                    t = st.steps
                    for i, f in enumerate(r.beam_force):
                        tok[i], parent[i] = f[min(t, len(f) - 1)], (i if n_src > 1 else 0)
                    eot_fin[:] = 0
                parents = st.advance(tok, parent, lp, cum_out, eot_score, eot_fin, elp_h[a:b])
                if st.done:
                    done += self._end(r)
                else:
                    pairs += self._fork(r.beam, parents)
        if pairs:
            ops.kv_copy_blocks(e.kv.k, e.kv.v, pairs)
        return done

    def _fork(self, g: BeamGroup, parents: list) -> list:
        """Re-parent ``g``'s sequences after a step: (source block, destination
        block) of every copy it needs."""
        e = self.e
        pool, bs = e.kv.pool, e.block_size
        while len(g.seqs) < len(parents):
            sid = e._next
            e._next += 1
            pool.add_seq(sid, [])
            g.seqs.append(sid)
        phys: list = [None] * len(parents)
        inherited = set()
        for i, p in enumerate(parents):
            if g.phys[p] not in inherited:     # the first child keeps the parent's sequence
                phys[i] = g.phys[p]
                inherited.add(g.phys[p])
        free = [s for s in g.seqs if s not in inherited]
        pairs = []
        for i, p in enumerate(parents):
            if phys[i] is not None:
                continue
            src, dst = g.phys[p], free.pop()
            n, have = pool.seq_len(src), pool.seq_len(dst)
            if have > n:
                pool.truncate(dst, n)
            elif have < n and pool.append(dst, n - have) is None:
                raise RuntimeError("STT KV cache out of blocks (beam search)")
            nb = -(-n // bs)
            pairs += list(zip(pool.block_table(src)[:nb], pool.block_table(dst)[:nb]))
            phys[i] = dst
            e.stats["beam_kv_copies"] += 1
        g.phys = phys
        return pairs

    def _end(self, r) -> list:
        """The window's search is over: the winner becomes the request's tokens
        and log-probabilities, the other sequences go back to the pool, and the
        engine finishes the window as it does a greedy one."""
        e = self.e
        g, r.beam = r.beam, None
        hyps, w = g.state.result()
        score = [s / max(1, sum(1 for x in t if x != e.eot)) for t, s, _ in hyps]
        order = sorted(range(len(hyps)), key=lambda i: -score[i])      # stable: the winner first
        r.tokens, r.logprobs = list(hyps[w][0]), list(hyps[w][2])
        r.step = len(r.tokens)
        r.hypotheses = [(list(hyps[i][0]), hyps[i][1]) for i in order]
        r.hypothesis_traces = [g.state.result_trace[i] for i in order]
        r.window_hypotheses.append(r.hypotheses)
        for sid in g.seqs:
            if sid != r.seq_id:
                e.kv.pool.free_seq(sid)
        f = e._finish(r)
        return [f] if f is not None else []

    def abort(self, r) -> None:
        """Free what ``r``'s group holds beyond ``r.seq_id`` (a failed batch)."""
        if r.beam is not None:
            for sid in r.beam.seqs:
                if sid != r.seq_id:
                    self.e.kv.pool.free_seq(sid)
            r.beam = None

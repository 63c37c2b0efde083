"""Step I/O of the captured decode steps, shared by ``LLMEngine`` and ``STTEngine``.

A decode-step graph exchanges its host data without copy-engine operations
(csrc/kernels/elementwise.hip, "pipelined decode: step I/O"): every graph is
``loqa_step_fetch`` -> step body -> ``loqa_step_publish[_lp[2]]``.

* The host stages a step's metadata in a pinned ring of ``STAGE_SLOTS`` rows;
  the fetch node reads the row of this launch into the graph's device buffers
  and takes every token whose ``src`` entry is >= 0 from ``last_tok[src]`` (a
  token the host has not seen yet: the pipelined decodes launch step j+1
  while step j runs).
* The publish node writes the sampled tokens (and their log-probabilities)
  into a pinned result ring of ``RES_SLOTS`` rows and into
  ``last_tok[row_slot]`` (padding rows write the trash slot, the table's last).
* A device counter of launched step graphs picks both rows; the host keeps
  the same number (``StepIO.step_no``), and both wrap at ``WRAP``.

``StepLayout`` is the flat layout of one graph's metadata (pure numpy),
``StepIO`` owns the rings and captures / stages / replays, ``stage_feeds``,
``fill_meta``, ``to_device`` and ``decode_buckets`` are the host loops the two
engines and their pipelines share.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import ops

DEV = -1   # feed placeholder: "the token this sequence sampled in its previous step"

# fields with one entry per token row; cu_q and block_tables have shapes of
# their own, every other field has one entry per sequence
_PER_TOKEN = ("tokens", "positions", "slots", "src")


def step_shapes(fields, B_pad: int, T_pad: int, max_blocks: int) -> dict:
    """``{field: shape}`` of an engine's int32 step fields, in its order."""
    own = {"cu_q": (B_pad + 1,), "block_tables": (B_pad, max_blocks)}
    return {f: (T_pad,) if f in _PER_TOKEN else own.get(f, (B_pad,)) for f in fields}


class StepLayout:
    """One graph's step metadata: int32 fields back to back in one flat block
    (``n32`` entries, ``offsets[field]``) and ``n64`` int64 logit rows in a
    second. ``step_fetch_kernel`` takes the first ``T`` entries as the tokens
    and finds their source slots at ``src_off``."""

    def __init__(self, shapes: dict, n64: int):
        if next(iter(shapes), None) != "tokens":
            raise ValueError("step layout: 'tokens' must be the first field (the fetch kernel "
                             "gathers device-fed tokens at the head of the block)")
        for f in ("src", "row_slot"):
            if f not in shapes:
                raise ValueError(f"step layout: field {f!r} is missing")
        self.shapes = {k: tuple(int(d) for d in s) for k, s in shapes.items()}
        self.offsets, off = {}, 0
        for k, s in self.shapes.items():
            self.offsets[k] = off
            off += int(np.prod(s))
        self.n32, self.n64 = off, int(n64)
        self.src_off = self.offsets["src"]

    def views(self, flat32, flat64) -> dict:
        """The fields as views of a flat int32 buffer, ``logit_idx`` of a flat
        int64 one (numpy staging rows and device tensors alike)."""
        out = {}
        for k, s in self.shapes.items():
            o = self.offsets[k]
            out[k] = flat32[o:o + int(np.prod(s))].reshape(s)
        out["logit_idx"] = flat64[: self.n64]
        return out


class StepIO:
    """The rings, the counters and the graphs' I/O nodes of one engine."""
    STAGE_SLOTS = 2     # step_fetch_kernel reads row (counter & 1)
    RES_SLOTS = 3       # result ring rows (>= steps in flight + 1)
    WRAP = 2 * RES_SLOTS    # both counters wrap here, as step_publish_kernel wraps *ctr
    WIDTH = 256         # result ring row: the most sequences (B_pad) of one step

    def __init__(self, device, largest: StepLayout, last_tok: torch.Tensor,
                 logprobs: bool | int = False):
        """``largest``: the layout of the engine's largest bucket (sizes the
        staging rows); ``last_tok``: the engine's last-token table, its last
        entry the trash slot; ``logprobs``: an f32 result ring beside the
        tokens'; ``2``: its rows carry two f32 values per sequence (the token's
        log-probability and a probed one), as two planes of ``WIDTH``."""
        if logprobs not in (False, True, 2):
            raise ValueError("logprobs: False, True or 2")
        self.lp_cols = int(logprobs)
        self.device = device
        self.n32, self.n64 = largest.n32, largest.n64
        self.last_tok, self.trash = last_tok, last_tok.numel() - 1
        # pinned for the device's zero-copy reads and writes (a host-only StepIO,
        # device "cpu", keeps plain memory: its rings and result() work the same)
        pin = (lambda t: t.pin_memory()) if torch.device(device).type == "cuda" else (lambda t: t)
        self.stage32 = pin(torch.zeros(self.STAGE_SLOTS, self.n32, dtype=torch.int32))
        self.stage64 = pin(torch.zeros(self.STAGE_SLOTS, self.n64, dtype=torch.int64))
        self.res = pin(torch.zeros(self.RES_SLOTS, self.WIDTH, dtype=torch.int32))
        lp_shape = (self.RES_SLOTS, self.WIDTH) if self.lp_cols < 2 else \
            (self.RES_SLOTS, 2, self.WIDTH)
        self.res_lp = pin(torch.zeros(lp_shape, dtype=torch.float32)) if logprobs else None
        self.ctr = torch.zeros(1, dtype=torch.int32, device=device)   # launched step graphs
        self.step_no = 0                                              # the host's copy of it
        self._res = self.res.numpy()
        self._res_lp = self.res_lp.numpy() if logprobs else None

    @classmethod
    def check_depth(cls, depth: int) -> None:
        """A pipeline keeping ``depth`` steps in flight reads a result row
        while the next ``depth`` launches write the following rows."""
        assert cls.RES_SLOTS >= depth + 1, "result ring too shallow for the pipeline depth"

    def capture(self, layout: StepLayout, T_pad: int, body, warm=None) -> dict:
        """One decode-step graph: fetch node, ``body(dev)`` (the sampled tokens
        of the first ``B_pad`` rows; with the log-prob ring ``(tokens,
        logprobs)``, with its two-value rows ``(tokens, logprobs, probe
        logprobs)``), publish node. ``dev`` are the graph's device buffers in
        ``layout``. ``warm(dev)``: what the warm-up runs instead of the body."""
        B_pad = layout.shapes["row_slot"][0]
        assert layout.shapes["tokens"] == (T_pad,)
        assert layout.n32 <= self.n32 and layout.n64 <= self.n64 and B_pad <= self.WIDTH, \
            "step bucket exceeds the staging / result rings"
        # all int32 metadata lives in ONE device buffer, int64 logit rows in a second
        d32 = torch.zeros(layout.n32, dtype=torch.int32, device=self.device)
        d64 = torch.zeros(layout.n64, dtype=torch.int64, device=self.device)
        dev = layout.views(d32, d64)
        dev["slots"].fill_(-1)
        dev["src"].fill_(-1)
        dev["row_slot"].fill_(self.trash)
        # warm up (allocator + kernels) on a side stream, then capture; the
        # warm-up runs the body only (the I/O nodes would advance the counter)
        s = torch.cuda.Stream(self.device)
        s.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(s):
            (warm or body)(dev)
        torch.cuda.current_stream(self.device).wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        lib = ops._lib
        k = lib.kernels()
        # thread-local capture: the other GPU worker thread keeps running
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            st = lib.stream_ptr(d32)
            lib.check(k.loqa_step_fetch(
                lib.ptr(d32), self.stage32.data_ptr(), layout.n32, self.n32, lib.ptr(d64),
                self.stage64.data_ptr(), layout.n64, self.n64, lib.ptr(self.ctr), T_pad,
                layout.src_off, lib.ptr(self.last_tok), st), "step_fetch")
            out = body(dev)
            if self.lp_cols == 2:
                lib.check(k.loqa_step_publish_lp2(
                    lib.ptr(out[0]), lib.ptr(out[1]), lib.ptr(out[2]), B_pad, self.res.data_ptr(),
                    self.WIDTH, self.res_lp.data_ptr(), 2 * self.WIDTH, self.WIDTH, self.RES_SLOTS,
                    lib.ptr(self.ctr), lib.ptr(dev["row_slot"]), lib.ptr(self.last_tok), st),
                    "step_publish_lp2")
            elif self.res_lp is not None:
                lib.check(k.loqa_step_publish_lp(
                    lib.ptr(out[0]), lib.ptr(out[1]), B_pad, self.res.data_ptr(), self.WIDTH,
                    self.res_lp.data_ptr(), self.WIDTH, self.RES_SLOTS, lib.ptr(self.ctr),
                    lib.ptr(dev["row_slot"]), lib.ptr(self.last_tok), st), "step_publish_lp")
            else:
                lib.check(k.loqa_step_publish(
                    lib.ptr(out), B_pad, self.res.data_ptr(), self.WIDTH, self.RES_SLOTS,
                    lib.ptr(self.ctr), lib.ptr(dev["row_slot"]), lib.ptr(self.last_tok), st),
                    "step_publish")
        # the staging rows in this graph's layout, built once (stage() per step
        # is one list index)
        host = [layout.views(self.stage32[i].numpy(), self.stage64[i].numpy())
                for i in range(self.STAGE_SLOTS)]
        return {"graph": graph, "dev": dev, "out": out, "layout": layout, "host": host}

    def stage(self, g: dict) -> dict:
        """Numpy views, in graph ``g``'s layout, of the staging row the NEXT
        step-graph launch reads. The row was last read by the step two
        launches back, so at most ``STAGE_SLOTS`` steps may be in flight."""
        return g["host"][self.step_no % self.STAGE_SLOTS]

    def replay(self, g: dict) -> int:
        """Launch a step graph whose staging row is filled; returns the result
        ring row its sampled tokens land in."""
        rslot = self.step_no % self.RES_SLOTS
        g["graph"].replay()
        self.step_no = (self.step_no + 1) % self.WRAP
        return rslot

    def result(self, rslot: int, B: int):
        """Copies of the first ``B`` tokens of result row ``rslot`` (once its
        step has finished); with the log-prob ring ``(tokens, logprobs)``, with
        its two-value rows ``(tokens, logprobs, probe logprobs)``."""
        toks = self._res[rslot, :B].copy()
        if self._res_lp is None:
            return toks
        if self.lp_cols == 2:
            return toks, self._res_lp[rslot, 0, :B].copy(), self._res_lp[rslot, 1, :B].copy()
        return toks, self._res_lp[rslot, :B].copy()


def stage_feeds(host: dict, feeds: list, slots: list, trash: int) -> None:
    """Write the sequences' ``feeds`` into a step's ``tokens`` / ``src`` and
    their ``last_tok`` slots into ``row_slot``. A ``DEV`` placeholder becomes
    token 0 with ``src`` = its sequence's slot (the fetch node takes the token
    from ``last_tok`` there); every other ``src`` entry is -1, padding tokens
    are 0 and padding rows point at the ``trash`` slot."""
    toks, src, row_slot = host["tokens"], host["src"], host["row_slot"]
    flat = [t for f in feeds for t in f]
    T = len(flat)
    toks[:T] = [0 if t == DEV else t for t in flat]
    toks[T:] = 0
    src[:T] = [sl if t == DEV else -1 for f, sl in zip(feeds, slots) for t in f]
    src[T:] = -1
    row_slot[: len(slots)] = slots
    row_slot[len(slots):] = trash


def fill_meta(pool, seq_ids: list, feeds: list, B_pad: int, T_pad: int, max_blocks: int,
              n64: int, out: dict | None = None, what: str = "KV cache") -> dict:
    """Host metadata of one step (``pool.step_meta``: positions, KV slots,
    query offsets, context lengths, block tables, logit rows) plus the fed
    tokens. ``out``: preallocated views (a staging row) filled in place and
    returned; else fresh arrays."""
    if out is None:
        out = {"tokens": np.zeros(T_pad, np.int32), "positions": np.zeros(T_pad, np.int32),
               "slots": np.full(T_pad, -1, np.int32), "cu_q": np.zeros(B_pad + 1, np.int32),
               "ctx_lens": np.zeros(B_pad, np.int32),
               "block_tables": np.zeros((B_pad, max_blocks), np.int32),
               "logit_idx": np.zeros(n64, np.int64)}
    tokens = out["tokens"]
    tokens.fill(0)
    T = sum(len(f) for f in feeds)
    if T:
        tokens[:T] = [t for f in feeds for t in f]
    rc = pool.step_meta(seq_ids, [len(f) for f in feeds], B_pad, T_pad, max_blocks,
                        out["positions"], out["slots"], out["cu_q"], out["ctx_lens"],
                        out["block_tables"], out["logit_idx"])
    if rc == -2:
        raise RuntimeError(f"{what} exhausted")
    if rc != 0:
        raise RuntimeError(f"step metadata failed ({rc})")
    return out


def to_device(host: dict, device: torch.device, dst: dict | None = None) -> dict:
    """Host arrays -> (pinned) -> ``device``; ``dst``: existing device tensors
    to copy into."""
    out = {}
    for k, a in host.items():
        t = torch.from_numpy(a)
        if device.type == "cuda":
            t = t.pin_memory()
        if dst is not None:
            dst[k].copy_(t, non_blocking=True)
            out[k] = dst[k]
        else:
            out[k] = t.to(device, non_blocking=True)
    return out


def decode_buckets(seq_buckets, max_seqs: int, step_tokens: int, max_q: int, ctx_step: int,
                   ctx_max: int) -> list:
    """Every (sequence, token, context) bucket a decode step of at most
    ``max_seqs`` sequences, ``step_tokens`` tokens and ``max_q`` tokens per
    sequence can fall into."""
    out = []
    b_max = next((b for b in seq_buckets if b >= max_seqs), seq_buckets[-1])
    for b in seq_buckets:
        if b > b_max:
            break
        t_min = ops.mpad_for(min(step_tokens, b // 2 + 1))   # T >= B > b/2
        t_max = ops.mpad_for(min(step_tokens, b * max_q))
        for t in ops.MPADS:
            if t > t_max:
                break
            if t < t_min:
                continue
            out += [(b, t, min(c, ctx_max)) for c in range(ctx_step, ctx_max + ctx_step, ctx_step)]
    return out

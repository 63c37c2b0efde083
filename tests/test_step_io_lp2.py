"""Step I/O with two f32 values per sequence (``StepIO(logprobs=2)`` over
``loqa_step_publish_lp2``): the token's log-probability and a probed one, as two
planes of a result-ring row.

A numpy model of ``step_fetch_kernel`` and the three publish kernels (the model
of ``tests/test_step_io_gpu.py`` with the second plane) is compared bitwise
with

* the host side alone on the CPU: ``StepIO.result`` over rings the model
  wrote (ring slot, the wrap at 6, the last-token table, trash rows);
* a real ``StepIO`` on the GPU with a trivial body, across the counter wrap,
  with device-fed tokens and two steps in flight - in all three modes, so the
  ``logprobs=False`` / ``True`` rings and the old entries are what they were.
"""
import numpy as np
import pytest
import torch

from loqa_hub_amd.engine.llm_engine import LLMEngine
from loqa_hub_amd.engine.step_io import DEV, StepIO, stage_feeds

MAX_BLOCKS = 2
N_SLOTS = 12            # sequence slots of last_tok; slot N_SLOTS is the trash slot
USED_SLOTS = 10         # slots 10, 11 are never a row's slot: they stay untouched
ORDER = [0, 1, 0, 1, 1, 0, 1, 0, 1]     # graph of every replay (see test_step_io_gpu.py)
PAIRS = {1, 4, 7}       # steps launched together with their successor, one wait


def lp_shape(mode):
    return (StepIO.RES_SLOTS, 2, StepIO.WIDTH) if mode == 2 else (StepIO.RES_SLOTS, StepIO.WIDTH)


class KernelModel:
    """What step_fetch_kernel and step_publish[_lp[2]]_kernel do to the buffers.
    ``mode``: False, True or 2, as ``StepIO(logprobs=...)``."""

    def __init__(self, mode, res=None, res_lp=None):
        self.mode = mode
        self.last_tok = np.zeros(N_SLOTS + 1, np.int32)
        self.ctr = 0
        self.res = np.zeros((StepIO.RES_SLOTS, StepIO.WIDTH), np.int32) if res is None else res
        self.res_lp = res_lp
        if mode and res_lp is None:
            self.res_lp = np.zeros(lp_shape(mode), np.float32)

    def fetch(self, lay, staged32, staged64):
        d32 = staged32.copy()
        for i in range(lay.shapes["tokens"][0]):
            sl = staged32[lay.src_off + i]
            if sl >= 0:
                d32[i] = max(self.last_tok[sl], 0)
        return lay.views(d32, staged64.copy())

    def publish(self, out, lp, lp2, row_slot):
        rslot = self.ctr % StepIO.RES_SLOTS
        n = out.size
        self.res[rslot, :n] = out
        if self.mode == 2:
            self.res_lp[rslot, 0, :n] = lp
            self.res_lp[rslot, 1, :n] = lp2
        elif self.mode:
            self.res_lp[rslot, :n] = lp
        for i, v in enumerate(out):
            self.last_tok[row_slot[i]] = v
        self.ctr = (self.ctr + 1) % (2 * StepIO.RES_SLOTS)
        return rslot

    def step(self, lay, staged32, staged64):
        dev = self.fetch(lay, staged32, staged64)
        out, lp, lp2 = body_np(dev, lay.shapes["row_slot"][0])
        return dev, out, lp, lp2, self.publish(out, lp, lp2, dev["row_slot"])


def body_np(dev, B_pad):
    out = dev["tokens"][:B_pad] - 5 + dev["positions"][:B_pad]
    f = out.astype(np.float32)           # all three exact in f32
    return out, f * np.float32(0.25) - np.float32(0.5), f * np.float32(-0.125) + np.float32(3.0)


def body_torch(dev, B_pad, mode):
    out = dev["tokens"][:B_pad] - 5 + dev["positions"][:B_pad]
    if not mode:
        return out
    f = out.float()
    return (out, f * 0.25 - 0.5, f * -0.125 + 3.0) if mode == 2 else (out, f * 0.25 - 0.5)


# ------------------------------------------------------------------ host side
def test_logprobs_argument():
    lay = LLMEngine.step_layout(8, 32, MAX_BLOCKS)
    last_tok = torch.zeros(N_SLOTS + 1, dtype=torch.int32)
    for mode in (False, True, 2):
        io = StepIO("cpu", lay, last_tok, logprobs=mode)
        assert io.res.shape == (StepIO.RES_SLOTS, StepIO.WIDTH) and io.res.dtype == torch.int32
        if not mode:
            assert io.res_lp is None
        else:
            assert tuple(io.res_lp.shape) == lp_shape(mode) and io.res_lp.dtype == torch.float32
            assert io.res_lp.is_contiguous()
        assert io.trash == N_SLOTS and io.step_no == 0
    for bad in (3, -1, 1.5, "2"):
        with pytest.raises(ValueError):
            StepIO("cpu", lay, last_tok, logprobs=bad)


@pytest.mark.parametrize("mode", [False, True, 2], ids=["tokens", "logprobs", "lp2"])
def test_result_reads_the_models_rings(mode):
    """The model's publish writes ``StepIO``'s own rings (as the kernel writes
    the pinned ones); ``result`` returns copies of the first B entries of the
    row the host's step number picked, over 2 * WRAP + 1 steps."""
    rng = np.random.default_rng(11)
    lay = LLMEngine.step_layout(8, 32, MAX_BLOCKS)
    io = StepIO("cpu", lay, torch.zeros(N_SLOTS + 1, dtype=torch.int32), logprobs=mode)
    model = KernelModel(mode, io.res.numpy(), io.res_lp.numpy() if mode else None)
    assert StepIO.WRAP == 6
    seen = []
    for step in range(2 * StepIO.WRAP + 1):
        B_pad = (4, 8)[step % 2]
        B = int(rng.integers(1, B_pad + 1))
        out = rng.integers(-3, 50, B_pad).astype(np.int32)
        lp = rng.standard_normal(B_pad).astype(np.float32)
        lp2 = rng.standard_normal(B_pad).astype(np.float32)
        slots = rng.permutation(USED_SLOTS)[:B].tolist()
        row_slot = np.array(slots + [io.trash] * (B_pad - B), np.int32)
        out[B:] = 7                               # padding rows: one value for the trash slot
        before = {k: v.copy() for k, v in (("res", model.res), ("lp", model.res_lp))
                  if v is not None}
        assert io.step_no == model.ctr
        rslot = io.step_no % StepIO.RES_SLOTS     # what replay() returns for this launch
        assert model.publish(out, lp, lp2, row_slot) == rslot == step % StepIO.RES_SLOTS
        io.step_no = (io.step_no + 1) % StepIO.WRAP
        seen.append(io.step_no)
        got = io.result(rslot, B)
        if not mode:
            assert isinstance(got, np.ndarray) and np.array_equal(got, out[:B])
        else:
            assert len(got) == (3 if mode == 2 else 2)
            assert np.array_equal(got[0], out[:B])
            assert got[1].dtype == np.float32 and got[1].tobytes() == lp[:B].tobytes()
            if mode == 2:
                assert got[2].dtype == np.float32 and got[2].tobytes() == lp2[:B].tobytes()
            # copies: a later step's write does not change them
            assert not any(np.shares_memory(g, io.res_lp.numpy()) for g in got[1:])
        # only this row changed, and only its first B_pad entries per plane
        other = [i for i in range(StepIO.RES_SLOTS) if i != rslot]
        assert np.array_equal(model.res[other], before["res"][other])
        assert np.array_equal(model.res[rslot, B_pad:], before["res"][rslot, B_pad:])
        if mode:
            assert model.res_lp[other].tobytes() == before["lp"][other].tobytes()
            assert model.res_lp[rslot, ..., B_pad:].tobytes() == \
                before["lp"][rslot, ..., B_pad:].tobytes()
        # last_tok: the sequences' slots and the trash slot
        assert model.last_tok[slots].tolist() == out[:B].tolist()
        if B < B_pad:
            assert model.last_tok[io.trash] == 7
    assert seen[StepIO.WRAP - 1] == 0 and seen[-1] == 1       # wrapped twice
    assert (model.last_tok[USED_SLOTS:N_SLOTS] == 0).all()


# ------------------------------------------------------------------ on the GPU
def stage_step(io, g, rng, fed_slots=()):
    """Fresh values in every field of the next staging row (as
    tests/test_step_io_gpu.py). Returns (B, the sequences' slots, copies of the
    staged int32 and int64 rows)."""
    lay, host = g["layout"], io.stage(g)
    B_pad, T_pad = lay.shapes["row_slot"][0], lay.shapes["tokens"][0]
    for f in lay.shapes:
        host[f][...] = rng.integers(0, 50, lay.shapes[f])
    host["logit_idx"][:] = rng.integers(0, 1 << 40, lay.n64)
    fed = list(fed_slots)[:B_pad]
    B = int(rng.integers(max(1, len(fed)), B_pad + 1))
    rest = [s for s in rng.permutation(USED_SLOTS).tolist() if s not in fed]
    slots = fed + rest[: B - len(fed)]
    feeds = [[DEV] for _ in fed] + [[DEV] if rng.random() < 0.3 else [int(rng.integers(0, 10))]
                                    for _ in range(B - len(fed))]
    stage_feeds(host, feeds, slots, io.trash)
    host["positions"][:] = rng.integers(0, 4, T_pad)
    host["positions"][B:B_pad] = int(rng.integers(0, 4))     # one value for the trash slot
    n = T_pad - B_pad
    host["tokens"][B_pad:] = rng.integers(0, 10, n)
    host["src"][B_pad:] = np.where(rng.random(n) < 0.5, rng.integers(0, N_SLOTS, n), -1)
    s = io.step_no % StepIO.STAGE_SLOTS
    return B, slots, io.stage32[s, : lay.n32].numpy().copy(), io.stage64[s, : lay.n64].numpy().copy()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [False, True, 2], ids=["tokens", "logprobs", "lp2"])
def test_step_io_protocol_gpu(mode):
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(5)
    last_tok = torch.zeros(N_SLOTS + 1, dtype=torch.int32, device=dev)
    io = StepIO(dev, LLMEngine.step_layout(8, 32, MAX_BLOCKS), last_tok, logprobs=mode)
    assert io.res.is_pinned() and (not mode or io.res_lp.is_pinned())
    graphs = []
    for B_pad, T_pad in ((4, 16), (8, 32)):
        lay = LLMEngine.step_layout(B_pad, T_pad, MAX_BLOCKS)
        graphs.append(io.capture(lay, T_pad, lambda d, b=B_pad: body_torch(d, b, mode)))
    torch.cuda.synchronize()
    assert int(io.ctr.item()) == 0 and io.step_no == 0 and not last_tok.any().item()
    model = KernelModel(mode)
    assert len(ORDER) == 2 * StepIO.RES_SLOTS + 3
    j = 0
    while j < len(ORDER):
        launched, fed = [], ()
        for k in range(j, j + (2 if j in PAIRS else 1)):
            g = graphs[ORDER[k]]
            B, slots, s32, s64 = stage_step(io, g, rng, fed)
            assert io.step_no == (model.ctr + len(launched)) % StepIO.WRAP
            launched.append((g, B, s32, s64, io.replay(g)))     # no wait in between
            fed = slots
        torch.cuda.synchronize()
        for g, B, s32, s64, rslot in launched:
            want_dev, out, lp, lp2, want_rslot = model.step(g["layout"], s32, s64)
            assert rslot == want_rslot
            got = io.result(rslot, B)
            if mode:
                assert len(got) == (3 if mode == 2 else 2)
                assert got[1].dtype == np.float32 and got[1].tobytes() == lp[:B].tobytes()
                if mode == 2:
                    assert got[2].dtype == np.float32 and got[2].tobytes() == lp2[:B].tobytes()
                got = got[0]
            assert np.array_equal(got, out[:B])
            for f, a in want_dev.items():
                assert np.array_equal(g["dev"][f].cpu().numpy(), a), f
        # every result row of every plane (untouched entries included), the
        # whole last-token table, both counters
        assert np.array_equal(io.res.numpy(), model.res)
        if mode:
            assert io.res_lp.numpy().tobytes() == model.res_lp.tobytes()
        assert np.array_equal(last_tok.cpu().numpy(), model.last_tok)
        assert int(io.ctr.item()) == model.ctr == io.step_no
        j += len(launched)
    assert (model.last_tok[USED_SLOTS:N_SLOTS] == 0).all()

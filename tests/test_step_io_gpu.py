"""The step I/O protocol on the GPU (``engine/step_io.py`` over
``loqa_step_fetch`` / ``loqa_step_publish[_lp]``): a real ``StepIO`` with a
trivial body, every buffer compared bitwise with a numpy model of the two
kernels - across the counter wrap, with both staging rows under both graphs,
device-fed tokens and two steps in flight. No model, no engine."""
import numpy as np
import pytest
import torch

from loqa_hub_amd.engine.llm_engine import LLMEngine
from loqa_hub_amd.engine.step_io import DEV, StepIO, stage_feeds

pytestmark = pytest.mark.gpu

MAX_BLOCKS = 2
N_SLOTS = 12            # sequence slots of last_tok; slot N_SLOTS is the trash slot
USED_SLOTS = 10         # slots 10, 11 are never a row's slot: they stay untouched
# graph of every replay: strict alternation would pin each graph to one staging
# row (both follow the step's parity), so the order flips once in the middle
ORDER = [0, 1, 0, 1, 1, 0, 1, 0, 1]
PAIRS = {1, 4, 7}       # steps launched together with their successor, one wait


class KernelModel:
    """What step_fetch_kernel and step_publish[_lp]_kernel do to the buffers."""

    def __init__(self, with_lp):
        self.last_tok = np.zeros(N_SLOTS + 1, np.int32)
        self.ctr = 0
        self.res = np.zeros((StepIO.RES_SLOTS, StepIO.WIDTH), np.int32)
        self.res_lp = np.zeros((StepIO.RES_SLOTS, StepIO.WIDTH), np.float32) if with_lp else None

    def step(self, lay, staged32, staged64):
        """One graph over the staged row: (device buffers after the fetch,
        the body's tokens, its log-probabilities, the result row)."""
        d32 = staged32.copy()
        for i in range(lay.shapes["tokens"][0]):
            sl = staged32[lay.src_off + i]
            if sl >= 0:
                d32[i] = max(self.last_tok[sl], 0)
        dev = lay.views(d32, staged64.copy())
        out, lp = body_np(dev, lay.shapes["row_slot"][0])
        rslot = self.ctr % StepIO.RES_SLOTS
        self.res[rslot, : out.size] = out
        if self.res_lp is not None:
            self.res_lp[rslot, : out.size] = lp
        for i, v in enumerate(out):
            self.last_tok[dev["row_slot"][i]] = v
        self.ctr = (self.ctr + 1) % (2 * StepIO.RES_SLOTS)
        return dev, out, lp, rslot


def body_np(dev, B_pad):
    out = dev["tokens"][:B_pad] - 5 + dev["positions"][:B_pad]
    return out, out.astype(np.float32) * np.float32(0.25) - np.float32(0.5)   # exact in f32


def body_torch(dev, B_pad, with_lp):
    out = dev["tokens"][:B_pad] - 5 + dev["positions"][:B_pad]
    return (out, out.float() * 0.25 - 0.5) if with_lp else out


def stage_step(io, g, rng, fed_slots=()):
    """Fresh values in every field of the next staging row: B single-token
    sequences in distinct slots (those in ``fed_slots`` first, device-fed),
    further token rows past the sequence rows, some of them device-fed too.
    Returns (B, the sequences' slots, copies of the staged int32 and int64 rows)."""
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
    # padding rows all write the trash slot: give them one value, so the slot's
    # content does not depend on the order of the kernel's stores
    host["positions"][B:B_pad] = int(rng.integers(0, 4))
    # token rows past the sequence rows: host tokens and device-fed ones
    # (any slot, the never-written ones included)
    n = T_pad - B_pad
    host["tokens"][B_pad:] = rng.integers(0, 10, n)
    host["src"][B_pad:] = np.where(rng.random(n) < 0.5, rng.integers(0, N_SLOTS, n), -1)
    s = io.step_no % StepIO.STAGE_SLOTS
    return B, slots, io.stage32[s, : lay.n32].numpy().copy(), io.stage64[s, : lay.n64].numpy().copy()


@pytest.mark.parametrize("with_lp", [False, True], ids=["tokens", "logprobs"])
def test_step_io_protocol(with_lp):
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(5)
    last_tok = torch.zeros(N_SLOTS + 1, dtype=torch.int32, device=dev)
    io = StepIO(dev, LLMEngine.step_layout(8, 32, MAX_BLOCKS), last_tok, logprobs=with_lp)
    assert io.trash == N_SLOTS
    graphs = []
    for B_pad, T_pad in ((4, 16), (8, 32)):
        lay = LLMEngine.step_layout(B_pad, T_pad, MAX_BLOCKS)
        graphs.append(io.capture(lay, T_pad, lambda d, b=B_pad: body_torch(d, b, with_lp)))
    assert graphs[0]["layout"].src_off != graphs[1]["layout"].src_off
    torch.cuda.synchronize()
    # capturing (and its warm-up of the body) runs no I/O node
    assert int(io.ctr.item()) == 0 and io.step_no == 0 and not last_tok.any().item()
    model = KernelModel(with_lp)
    assert len(ORDER) == 2 * StepIO.RES_SLOTS + 3
    negatives = clamped = 0
    j = 0
    while j < len(ORDER):
        launched, fed = [], ()
        for k in range(j, j + (2 if j in PAIRS else 1)):
            g = graphs[ORDER[k]]
            B, slots, s32, s64 = stage_step(io, g, rng, fed)
            assert io.step_no == (model.ctr + len(launched)) % StepIO.WRAP
            launched.append((g, B, s32, s64, io.replay(g)))     # no wait in between
            fed = slots                     # the pair's second step is fed from the first
        torch.cuda.synchronize()
        for g, B, s32, s64, rslot in launched:
            lay = g["layout"]
            src = s32[lay.src_off:lay.src_off + lay.shapes["tokens"][0]]
            clamped += int(((src >= 0) & (model.last_tok[np.maximum(src, 0)] < 0)).sum())
            want_dev, out, lp, want_rslot = model.step(lay, s32, s64)
            negatives += int((out < 0).sum())
            assert rslot == want_rslot
            got = io.result(rslot, B)
            if with_lp:
                assert got[1].dtype == np.float32 and got[1].tobytes() == lp[:B].tobytes()
                got = got[0]
            assert np.array_equal(got, out[:B])      # the first step of a pair: row intact
            for f, a in want_dev.items():           # the graph's device buffers, logit_idx included
                assert np.array_equal(g["dev"][f].cpu().numpy(), a), f
            assert np.array_equal(g["dev"]["logit_idx"].cpu().numpy(), s64)
        # every result row (the other rows unchanged), the whole last-token
        # table (untouched slots and the trash slot included), both counters
        assert np.array_equal(io.res.numpy(), model.res)
        if with_lp:
            assert io.res_lp.numpy().tobytes() == model.res_lp.tobytes()
        assert np.array_equal(last_tok.cpu().numpy(), model.last_tok)
        assert int(io.ctr.item()) == model.ctr == io.step_no
        j += len(launched)
    assert (model.last_tok[USED_SLOTS:N_SLOTS] == 0).all()
    # the run exercised what it is meant to: negative samples, and the fetch
    # clamp max(last_tok, 0) on a device-fed token
    assert negatives > 0 and clamped > 0

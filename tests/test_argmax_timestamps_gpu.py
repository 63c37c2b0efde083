"""``loqa_masked_argmax_ts`` (``masked_argmax_kernel<.., 3>`` +
``argmax_finalize_kernel<3>``, ``csrc/kernels/elementwise.hip``) against the
rules of ``ops.reference`` evaluated in fp64 on the stored logit values, and
``STTEngine(timestamps=True)`` on the GPU.

**Shapes.** V = 520 (one workgroup, a tail that is no whole vector group),
8232 (two chunks, the timestamp range 8180 .. 8219 across the 8192 boundary)
and 51866 (Whisper's layout, 7 chunks); bf16 and f32; a padded row stride (the
vector path) and an odd one (the scalar path).

**Rows.** Six per launch: the four state classes (text after text, a closed
pair, a lone timestamp, no timestamp yet), a rule-off probing row and a
window's first token; ``DRAWS`` launches per case on fresh logits.

**Margin.** ``d = (lseT - lseA) - (xt - lseA)`` in fp64 per ruled row. An f32
scan may decide a row with ``|d| < 1e-3`` either way, so such rows are left
out of the index / state / log-probability checks; ``test_margin_budget``
checks on the CPU that they are at most 5 % of the generated ruled rows.

**Log-probability bound.** ``tests/test_argmax_logprob.py``'s ``bound(V,
dtype)``, derived there for the same scan (the winner's class is one more
online sum of the same depth; the logits here lie within its R).
"""
import math

import numpy as np
import pytest
import torch
from test_argmax_logprob import R, bound

from loqa_hub_amd import ops
from loqa_hub_amd.engine.stt_engine import N_SAMPLES, STTEngine, STTRequest
from loqa_hub_amd.models.configs import whisper_config
from loqa_hub_amd.ops import reference as ref
from loqa_hub_amd.ops.reference import pack_mask

NINF = float("-inf")
MARGIN = 1e-3
DRAWS = 4
# (V, ts_begin, ts_count, eot, shift of the timestamp logits so that both classes win)
SHAPES = {520: (500, 20, 480, 1.5), 8232: (8180, 40, 8100, 2.5), 51866: (50365, 1501, 50257, 0.0)}
MAXI = 12


def _ld(V, kind):
    if kind == "odd":              # ld % 8 != 0 and ld % 4 != 0: the scalar path
        return (V + 3) | 1
    ld = -(-V // 64) * 64          # the lm_head GEMM's padded row
    return ld if ld > V else ld + 64


def _states(ts_count):
    k = ts_count // 3
    return [ref.ts_state_pack(k, False, True),     # text after text: timestamps from k + 1
            ref.ts_state_pack(k, True, True),      # a closed pair: no timestamp
            ref.ts_state_pack(k, True, False),     # a lone timestamp: from k, nothing below eot
            ref.ts_state_pack(-1, False, False)]   # no timestamp yet


_CACHE: dict = {}


def make_case(V, dtype, ld_kind, draw):
    """CPU tensors of one launch, built once per key and shared by every test:
    the [B + 2, ld] buffer (hostile outside [:B, :V]), the mask table and rows,
    probe, ctl, the state table before the launch, row_slot, and the fp64
    expectation per row: (idx, logprob, d, next word)."""
    key = (V, dtype, ld_kind, draw)
    if key in _CACHE:
        return _CACHE[key]
    tsb, tsc, eot, shift = SHAPES[V]
    B = 6
    g = torch.Generator().manual_seed(7 * V + 100 * draw + (dtype == torch.bfloat16))
    ld = _ld(V, ld_kind)
    x = (torch.randn(B, V, generator=g) * 3).clamp_(-12, 12)
    x[:, tsb:tsb + tsc] += shift
    assert float(x.abs().max()) <= R                # the bound's range of logits
    x = x.to(dtype)
    # row 0 of the table: a suppress mask (half the text, EOT, no other special,
    # no timestamp: ruled rows must ignore those bits); row 1: a few columns
    bits = torch.zeros(2, V, dtype=torch.bool)
    bits[0, :eot] = torch.rand(eot, generator=g) < 0.5
    bits[0, eot] = True
    bits[1, torch.randint(V, (8,), generator=g)] = True
    mask = pack_mask(bits)
    rows = torch.tensor([0, 0, 0, 0, 1, 0], dtype=torch.int32)
    probe = torch.tensor([5, -1, -1, -1, V - 1, -1], dtype=torch.int32)
    ctl = torch.tensor([2, 2, 2, 2, 0, 1], dtype=torch.int32)
    SENT = -77
    state = torch.full((12,), SENT, dtype=torch.int32)     # sentinels in the unused slots
    slot = torch.tensor([2, 9, 4, 7, 11, 5], dtype=torch.int32)   # row 4 (ctl 0): the last slot
    for s, w in zip(slot[:4].tolist(), _states(tsc)):
        state[s] = w
    hostile = 40.0                                   # far above every allowed logit
    buf = torch.full((B + 2, ld), hostile).to(dtype)
    buf[:B, :V] = x
    xs = buf[:B, :V].double()
    want = []
    for b in range(B):
        c = int(ctl[b])
        if c == 0:
            want.append(None)
            continue
        word = int(state[int(slot[b])])
        text_ok, lo, hi = ref.ts_allowed(word, c, tsc, MAXI)
        okx = bits[int(rows[b])].clone()
        okx[tsb:] = False
        okx[: (tsb, eot, 0)[text_ok]] = False
        okt = torch.zeros(V, dtype=torch.bool)
        okt[tsb + lo:tsb + hi + 1] = True
        xx, xt = xs[b].masked_fill(~okx, NINF), xs[b].masked_fill(~okt, NINF)
        lse_a = torch.logsumexp(xs[b].masked_fill(~(okx | okt), NINF), dim=-1)
        lse_t = torch.logsumexp(xt, dim=-1)
        any_x, any_t = bool(okx.any()), bool(okt.any())
        d = float((lse_t - lse_a) - (xx.max() - lse_a)) if any_x and any_t else math.inf
        fire = any_t and (not any_x or d > 0)
        row, lse = (xt, lse_t) if fire else (xx, lse_a)
        w = int(row.argmax())
        want.append((w, float(row[w] - lse), d, ref.ts_state_next(word, c, w, tsb)))
    out = dict(buf=buf, mask=mask, rows=rows, probe=probe, ctl=ctl, state=state, slot=slot,
               want=want, B=B, sent=SENT)
    _CACHE[key] = out
    return out


CASES = [(V, dt, ld) for V in SHAPES for dt in (torch.float32, torch.bfloat16)
         for ld in ("pad64", "odd")]
IDS = [f"{V}-{'bf16' if dt == torch.bfloat16 else 'f32'}-{ld}" for V, dt, ld in CASES]


def test_margin_budget():
    """CPU: the rows the margin leaves out are at most 5 % of the ruled rows,
    and both outcomes of the mass rule are well represented."""
    n = out = fired = contested = 0
    for V, dt, ld in CASES:
        if ld == "odd":
            continue                    # the same logits as pad64
        for draw in range(DRAWS):
            for w in make_case(V, dt, "pad64", draw)["want"]:
                if w is None:
                    continue
                n += 1
                out += abs(w[2]) < MARGIN
                if math.isfinite(w[2]):
                    contested += 1
                    fired += w[2] > 0
    print(f"ruled rows {n}, left out {out}, contested {contested}, fired {fired}")
    assert n == 5 * DRAWS * 6 and out <= 0.05 * n
    assert 0.2 * contested <= fired <= 0.8 * contested


def _launch(c, V, dev="cuda"):
    d = torch.device(dev)
    tsb, tsc, eot, _ = SHAPES[V]
    view = c["buf"].to(d)[:c["B"], :V]
    assert view.stride(0) == c["buf"].shape[1]
    state = c["state"].to(d)
    args = (view, c["mask"].to(d), c["rows"].to(d), c["probe"].to(d), c["ctl"].to(d), state,
            c["slot"].to(d), tsb, tsc, eot, MAXI)
    idx, lp, plp = ops.masked_argmax_timestamps(*args)
    return args, idx.cpu(), lp.cpu(), plp.cpu(), state.cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("V,dtype,ld_kind", CASES, ids=IDS)
def test_kernel_against_the_rules_in_fp64(V, dtype, ld_kind):
    tsb = SHAPES[V][0]
    kept = 0
    for draw in range(DRAWS):
        c = make_case(V, dtype, ld_kind, draw)
        args, idx, lp, plp, state = _launch(c, V)
        # rule-off rows: bitwise the probe op on the same inputs; their slot untouched
        p_idx, p_lp, p_plp = (t.cpu() for t in ops.masked_argmax_logprob_probe(*args[:4]))
        want_state = c["state"].clone()
        for b, w in enumerate(c["want"]):
            if w is None:
                assert int(idx[b]) == int(p_idx[b])
                assert lp[b].view(torch.int32) == p_lp[b].view(torch.int32)
                continue
            s = int(c["slot"][b])
            if abs(w[2]) < MARGIN:
                want_state[s] = state[s]         # either decision: not checked
                continue
            kept += 1
            err = abs(float(lp[b]) - w[1])
            print(f"V={V} {dtype} {ld_kind} draw {draw} row {b}: idx {int(idx[b])} want {w[0]} "
                  f"d {w[2]:.3e} lp err {err:.3e} bound {bound(V, dtype):.3e}")
            assert int(idx[b]) == w[0], (b, int(idx[b]), w)
            assert err <= bound(V, dtype), (b, err, bound(V, dtype))
            want_state[s] = w[3]
        # the probe is the mask- and rule-free log-softmax on every row
        assert torch.equal(plp.view(torch.int32), p_plp.view(torch.int32))
        assert float(plp[0]) < 0.0 and float(plp[4]) < 0.0 and plp[1:4].tolist() == [0.0] * 3
        # hostile memory: only the ruled rows' slots changed, the sentinels
        # (unused slots, and the rule-off row's) are intact
        assert torch.equal(state, want_state), (state, want_state)
        assert int(state[11]) == c["sent"] and (state[[0, 1, 3, 6, 8, 10]] == c["sent"]).all()
        # bitwise repeatable, from the same state
        _, idx2, lp2, plp2, state2 = _launch(c, V)
        assert torch.equal(idx, idx2) and torch.equal(state, state2)
        assert torch.equal(lp.view(torch.int32), lp2.view(torch.int32))
    assert kept >= 4 * DRAWS


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_decision_edges_bitwise(dtype):
    from test_argmax_timestamps import run_edges
    run_edges("cuda", dtype)


def chain_case(V):
    """The device-fed chain's inputs and the reference loop's results, built
    once on the CPU: 16 steps of fixed logits for two sequences and two padding
    rows (ctl 0, the trash slot). A step whose decision lies inside the margin
    would void the comparison, so the seed is one where none does (asserted
    here, and on the CPU by ``test_chain_seeds_clear_the_margin``)."""
    key = ("chain", V)
    if key in _CACHE:
        return _CACHE[key]
    tsb, tsc, eot, shift = SHAPES[V]
    B, STEPS, SENT = 4, 16, -99
    g = torch.Generator().manual_seed(5 + V)
    xs = (torch.randn(STEPS, B, V, generator=g) * 3).clamp_(-12, 12)
    xs[:, :, tsb:tsb + tsc] += shift
    bits = torch.zeros(1, V, dtype=torch.bool)
    bits[0, :eot] = torch.rand(eot, generator=g) < 0.5
    bits[0, eot] = True
    mask = pack_mask(bits)
    rows = torch.zeros(B, dtype=torch.int32)
    probe = torch.full((B,), -1, dtype=torch.int32)
    slot = torch.tensor([3, 1, 5, 5], dtype=torch.int32)      # rows 2, 3: padding, the trash slot
    ctls = [torch.tensor([1 if s == 0 else 2, 1 if s == 0 else 2, 0, 0], dtype=torch.int32)
            for s in range(STEPS)]
    state0 = torch.full((6,), SENT, dtype=torch.int32)
    st = state0.clone()
    want = []
    for s in range(STEPS):
        for b in (0, 1):
            word = int(st[int(slot[b])])
            text_ok, lo, hi = ref.ts_allowed(word, int(ctls[s][b]), tsc, MAXI)
            okx = bits[0].clone()
            okx[tsb:] = False
            okx[: (tsb, eot, 0)[text_ok]] = False
            x64 = xs[s, b].double()
            if okx.any() and lo <= hi:
                lt = torch.logsumexp(x64[tsb + lo:tsb + hi + 1], dim=-1)
                assert abs(float(lt - x64.masked_fill(~okx, NINF).max())) >= MARGIN, (s, b)
        idx, _, _ = ref.masked_argmax_timestamps(xs[s], mask, rows, probe, ctls[s], st, slot, tsb,
                                                 tsc, eot, MAXI)
        want.append(idx[:2].clone())
    out = dict(xs=xs, mask=mask, rows=rows, probe=probe, slot=slot, ctls=ctls, state0=state0,
               final=st, want=want, sent=SENT, steps=STEPS)
    _CACHE[key] = out
    return out


@pytest.mark.parametrize("V", [520, 51866])
def test_chain_seeds_clear_the_margin(V):
    c = chain_case(V)
    tsb, _, eot, _ = SHAPES[V]
    toks = [[int(w[b]) for w in c["want"]] for b in (0, 1)]
    assert all(tsb <= t[0] <= tsb + MAXI for t in toks)
    assert any(t >= tsb for tk in toks for t in tk[1:]) and any(t < eot for tk in toks for t in tk)
    assert c["final"][[0, 2, 4, 5]].tolist() == [c["sent"]] * 4


@pytest.mark.gpu
@pytest.mark.parametrize("V", [520, 51866])
def test_device_fed_chain(V):
    """16 launches on one stream whose logits are fixed in advance: only
    ``ts_state`` carries information from one launch to the next and the host
    reads nothing in between. The final tokens and state are the reference
    loop's, two runs agree bitwise, padding rows wrote nothing."""
    c = chain_case(V)
    tsb, tsc, eot, _ = SHAPES[V]
    d = torch.device("cuda")
    STEPS = c["steps"]
    runs = []
    for _ in range(2):
        state = c["state0"].to(d)
        dx, dm, dr = c["xs"].to(d), c["mask"].to(d), c["rows"].to(d)
        dp, dsl = c["probe"].to(d), c["slot"].to(d)
        dctl = [t.to(d) for t in c["ctls"]]
        torch.cuda.synchronize()
        outs = [ops.masked_argmax_timestamps(dx[s], dm, dr, dp, dctl[s], state, dsl, tsb, tsc, eot,
                                             MAXI) for s in range(STEPS)]   # no host read between
        torch.cuda.synchronize()
        runs.append(([o[0].cpu() for o in outs], [o[1].cpu() for o in outs], state.cpu()))
    (i1, l1, s1), (i2, l2, s2) = runs
    for s in range(STEPS):
        assert torch.equal(i1[s][:2], c["want"][s]), (s, i1[s], c["want"][s])
        assert torch.equal(i1[s], i2[s]) and torch.equal(l1[s].view(torch.int32),
                                                         l2[s].view(torch.int32))
    assert torch.equal(s1, c["final"]) and torch.equal(s1, s2)
    assert s1[[0, 2, 4, 5]].tolist() == [c["sent"]] * 4  # the trash slot included: nothing written


# ---------------------------------------------------------------------- engine
CFG = whisper_config("test-whisper")


@pytest.fixture(scope="module")
def weights():
    from loqa_hub_amd.models.whisper import WhisperWeights
    return WhisperWeights(CFG, torch.device("cuda", 0), seed=2)


@pytest.fixture(scope="module")
def cpu_weights():
    from loqa_hub_amd.models.whisper import WhisperWeights
    return WhisperWeights(CFG, torch.device("cpu"), seed=2)


def _pcms():
    rng = np.random.default_rng(1)
    out = [(rng.standard_normal(n) * 3000).astype(np.int16)
           for n in (16000, 48000, 30000, 31 * 16000)]
    assert len(out[3]) > N_SAMPLES
    return out


def _run(eng, pipelined=False):
    """Three requests arrive one step apart, then the 31 s one (two windows)
    once two slots are free: the scheduler's loop without its thread, so the
    arrivals fall on the same steps in every run. ``pipelined``: through the
    two-deep ``STTPipeline``, else one synchronous step at a time."""
    from loqa_hub_amd.engine.stt_pipeline import STTPipeline
    reqs = [STTRequest(p, max_new_tokens=12) for p in _pcms()]
    pl = STTPipeline(eng) if pipelined else None
    pending, live, free = list(reqs), [], list(range(eng.max_batch))
    while pending or live:
        if pending and eng.rows_needed(pending[:1]) <= len(free):
            r = pending.pop(0)
            eng._admit([r], [free.pop(0) for _ in range(eng.rows_needed([r]))])
            if pl is not None:
                pl.admit(r)
            live.append(r)
        for r in (pl.pump(live) if pl is not None else eng._decode_once(live)) if live else []:
            free = sorted(free + r.slots)
        live = [r for r in live if r.t_done == 0.0]
    if pl is not None:
        pl.drain()
    if eng.is_gpu:
        torch.cuda.synchronize()
    return reqs


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [{}, {"language": "auto", "no_speech": True}],
                         ids=["plain", "probing"])
def test_engine_paths_agree(weights, kw):
    """The eager-launch step, the captured synchronous step, the pipeline
    (captured, and through ``_launch_sync`` with no graph) take the same steps
    on the same kernels: bitwise equal. The CPU engine runs the fp32 reference
    on an fp32 decoder, so it is held to the same well-formedness, not to the
    GPU's bf16 logits."""
    mk = lambda **k: STTEngine(CFG, "cuda", seed=2, max_batch=4, weights=weights, timestamps=True,
                               **kw, **k)
    eager = _run(mk(use_graphs=False))
    graph = _run(mk())
    warm = mk()
    assert warm.warmup_graphs() > 0 and warm._graphs_frozen
    plain = STTEngine(CFG, "cuda", seed=2, max_batch=4, weights=weights, **kw)
    plain.warmup_graphs()
    assert set(warm._graphs) == set(plain._graphs)          # the same bucket set
    keys = set(warm._graphs)
    piped = _run(warm, pipelined=True)
    assert set(warm._graphs) == keys and warm.stats["pl_steps"] > 0 and warm.stats["pl_spec"] > 0
    frozen = mk()
    frozen._graphs_frozen = True
    synced = _run(frozen, pipelined=True)
    assert frozen._graphs == {} and frozen.stats["pl_steps"] == 0
    b, eot = warm.ts_begin, warm.eot
    for e, g, p, s in zip(eager, graph, piped, synced):
        assert e.tokens == g.tokens == p.tokens == s.tokens and len(e.tokens) > 0
        assert e.logprobs == g.logprobs == p.logprobs == s.logprobs
        assert len(e.logprobs) == len(e.tokens)
        assert e.segments == g.segments == p.segments == s.segments
        assert e.text == g.text == p.text == s.text
        assert e.open_segments == g.open_segments == p.open_segments == s.open_segments
        assert e.avg_logprob == g.avg_logprob == p.avg_logprob == s.avg_logprob
        assert e.no_speech_probs == g.no_speech_probs == p.no_speech_probs == s.no_speech_probs
        assert b <= e.tokens[0] <= b + warm.max_initial
        stamps = [t for t in e.tokens if t >= b]
        assert stamps == sorted(stamps)
        for a_, b_, text in e.segments or []:
            assert 0.0 <= a_ <= b_ <= e.n_samples / 16000 and "<|" not in text
    assert [r.windows for r in eager] == [1, 1, 1, 2]


@pytest.mark.gpu
def test_cpu_engine_takes_the_same_steps(weights, cpu_weights):
    """The CPU engine stages the same control words and reaches the same
    decisions from the same logits: the GPU engine's logits of every step,
    replayed through the CPU reference with the CPU engine's own staging,
    give the GPU engine's tokens."""
    gpu = STTEngine(CFG, "cuda", seed=2, max_batch=4, weights=weights, timestamps=True,
                    use_graphs=False)
    taps = []
    sample = gpu._sample

    def tap(logits, dev):
        out = sample(logits, dev)
        taps.append((logits.float().cpu(), {k: dev[k].cpu() for k in
                                            ("mask_row", "probe", "ts_ctl", "row_slot")},
                     tuple(o.cpu() for o in out)))
        return out
    gpu._sample = tap
    reqs = [STTRequest(p, max_new_tokens=12) for p in _pcms()[:3]]
    gpu.transcribe(reqs)
    cpu = STTEngine(CFG, "cpu", seed=2, max_batch=4, weights=cpu_weights, timestamps=True)
    assert (cpu.ts_begin, cpu.ts_count, cpu.eot, cpu.max_initial, cpu.sot) == \
        (gpu.ts_begin, gpu.ts_count, gpu.eot, gpu.max_initial, gpu.sot)
    state = torch.zeros_like(cpu.ts_state)
    agree = n = 0
    for logits, dev, (idx, lp, _) in taps:
        B = logits.shape[0]
        before = state.clone()
        ci, cl, _ = ops.masked_argmax_timestamps(
            logits, cpu._sup, dev["mask_row"][:B], dev["probe"][:B], dev["ts_ctl"][:B], state,
            dev["row_slot"][:B], cpu.ts_begin, cpu.ts_count, cpu.eot, cpu.max_initial)
        for b in range(B):
            if int(dev["ts_ctl"][b]) == 0:
                continue
            n += 1
            if int(ci[b]) == int(idx[b]):
                agree += 1
                assert abs(float(cl[b]) - float(lp[b])) <= bound(CFG.vocab_size, torch.bfloat16)
            else:       # an f32 near-tie: follow the GPU's token so the chain stays comparable
                s = int(dev["row_slot"][b])
                state[s] = ref.ts_state_next(int(before[s]), int(dev["ts_ctl"][b]), int(idx[b]),
                                             cpu.ts_begin)
    assert n > 20 and agree >= n - 1, (agree, n)
    assert torch.equal(state, gpu.ts_state.cpu())

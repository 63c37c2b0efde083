"""``loqa_masked_argmax_sample`` (``masked_argmax_kernel<.., 4>`` +
``argmax_finalize_kernel<4>``, ``csrc/kernels/elementwise.hip``) and
``loqa_gumbel_noise`` on the GPU.

**Noise bound.** ``g = -logf(-logf(u))`` for an exact ``u`` (the integer part is
bitwise the host's, ``ops.reference.gumbel_uniform``). HIP's math API reference
gives the device ``logf`` a maximum error in ulp; that document is not part of
every ROCm install, so the figure used is the budget this suite already holds
the device ``logf`` / ``expf`` to, 2 ulp (``tests/test_argmax_logprob.py``, which
cites the reference's own figure as 1). One ulp is at most ``2**-23`` of the
value, so the first ``logf`` returns ``w (1 + e)`` with ``|e| <= 2**-22``; the
negation is exact. ``-log(w (1 + e)) = -log(w) - log1p(e)``: that relative
error of ``w`` is an absolute error of at most ``2**-22 (1 + 2**-22)`` in ``g``,
whatever ``w`` is. The second ``logf`` adds 2 ulp of its own result. Against the
fp64 value of the same ``u`` (whose own error, 1e-16 relative, is far below)::

    |g_device - g_fp64| <= 2**-22 (1 + 2**-22) + 2 ulp_f32(|g_fp64|)

At ``|g| <= 16.7`` this is at most 4.1e-6.

**Draw, bit for bit.** The device's noise, read back through
``ops.gumbel_noise`` (the same ``__device__`` function the kernel draws with),
is handed to ``ops.reference.masked_argmax_sample(..., noise=)``, which forms the
key ``x + T g`` in fp64 and rounds it once to f32 as the kernel's ``fmaf``
does: the index and the state word are equal, the log-probability (against
fp64) within ``tests/test_argmax_logprob.py``'s ``bound(V, dtype)``. The rows
that ``tests/test_argmax_sample.py`` describes as left out (two best keys within
4 ulp, mass-rule margin below 1e-3) are not compared; they are at most 5 %.

**Shapes** and the seven rows of a launch: ``test_argmax_sample.make_case``.
"""
import numpy as np
import pytest
import torch
from test_argmax_logprob import bound
from test_argmax_sample import CASE_MAXI as MAXI
from test_argmax_sample import (CASES, DRAWS, IDS, N_ROWS, RULE_OFF, chi_square, dist_rule_off,
                                dist_ruled, expect, make_case)
from test_argmax_timestamps import TSB
from test_argmax_timestamps_gpu import SHAPES

from loqa_hub_amd import ops
from loqa_hub_amd.ops import reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"


def noise_bound(g64: np.ndarray) -> np.ndarray:
    return 2.0 ** -22 * (1 + 2.0 ** -22) + \
        2.0 * np.spacing(np.abs(g64).astype(np.float32)).astype(np.float64)


@pytest.mark.parametrize("V", [520, 8232])
def test_noise_against_fp64(V):
    rng = torch.tensor([ref.key_i32(ref.sample_key(V, 0, 1, i)) for i in range(5)] + [0, -1],
                       dtype=torch.int32)
    g = ops.gumbel_noise(rng.to(DEV), V)
    assert g.shape == (7, V) and g.dtype == torch.float32
    u = ref.gumbel_uniform(ref.gumbel_hash(rng, V)).double().numpy()
    g64 = -np.log(-np.log(u))
    err = np.abs(g.cpu().double().numpy() - g64)
    b = noise_bound(g64)
    print(f"V={V}: max err {err.max():.3e}, max err / bound {float((err / b).max()):.3f}, "
          f"g in [{g64.min():.2f}, {g64.max():.2f}]")
    assert bool((err <= b).all())
    assert float(b.max()) < 4.1e-6
    # rows differ, a launch repeats bitwise, and the host's f32 noise is close
    assert not torch.equal(g[0], g[1])
    assert torch.equal(g.view(torch.int32), ops.gumbel_noise(rng.to(DEV), V).view(torch.int32))
    assert float((g.cpu() - ref.gumbel_noise(rng, V)).abs().max()) < 1e-5


def _launch(c, V, temp=None, ctl="case"):
    d = torch.device(DEV)
    tsb, tsc, eot, _ = SHAPES[V]
    view = c["buf"].to(d)[:c["B"], :V]
    assert view.stride(0) == c["buf"].shape[1]
    state = c["state"].to(d)
    t = c["temp"] if temp is None else temp
    args = [view, c["mask"].to(d), c["rows"].to(d), c["probe"].to(d), c["ctl"].to(d), state,
            c["slot"].to(d), tsb, tsc, eot, MAXI, t.to(d), c["rng"].to(d)]
    if ctl is None:
        args[4:11] = [None, None, None, 0, 0, 0, 0]
    idx, lp, plp = ops.masked_argmax_sample(*args)
    return args, idx.cpu(), lp.cpu(), plp.cpu(), state.cpu()


@pytest.mark.parametrize("V,dtype,ld_kind", CASES, ids=IDS)
def test_draw_bit_for_bit(V, dtype, ld_kind):
    kept = skipped = 0
    for draw in range(DRAWS):
        c = make_case(V, dtype, ld_kind, draw)
        noise = ops.gumbel_noise(c["rng"].to(DEV), V).cpu()
        want, want_plp = expect(c, noise)
        args, idx, lp, plp, state = _launch(c, V)
        want_state = c["state"].clone()
        for b, (w_idx, w_lp, nxt, skip) in enumerate(want):
            s = int(c["slot"][b])
            if skip:
                skipped += 1
                want_state[s] = state[s]
                continue
            err = abs(float(lp[b]) - w_lp) if w_idx >= 0 else 0.0
            print(f"V={V} {dtype} {ld_kind} draw {draw} row {b}: idx {int(idx[b])} want {w_idx} "
                  f"lp err {err:.3e} bound {bound(V, dtype):.3e}")
            assert int(idx[b]) == w_idx, (b, int(idx[b]), w_idx)
            if w_idx < 0:
                assert float(lp[b]) == float("-inf")
            else:
                kept += 1
                assert err <= bound(V, dtype), (b, err)
            if nxt is not None:
                want_state[s] = nxt
        # the probe ignores mask, rules and temperature: bitwise the probe op's
        p_plp = ops.masked_argmax_logprob_probe(*args[:4])[2].cpu()
        assert torch.equal(plp.view(torch.int32), p_plp.view(torch.int32))
        assert float(plp[1]) < 0.0 and float(plp[4]) < 0.0 and plp[[0, 2, 3, 5, 6]].tolist() == [0.0] * 5
        assert float((plp - want_plp).abs().max()) < 1e-4
        # hostile memory: only the ruled rows' slots changed; the rule-off row's
        # slot (11), the nothing-allowed row's (1) and the unused ones are intact
        assert torch.equal(state, want_state), (state, want_state)
        assert int(state[11]) == c["sent"] and int(state[1]) == int(c["state"][1])
        assert (state[[0, 3, 6, 8, 10]] == c["sent"]).all()
        # bitwise repeatable, from the same state
        _, idx2, lp2, plp2, state2 = _launch(c, V)
        assert torch.equal(idx, idx2) and torch.equal(state, state2)
        assert torch.equal(lp.view(torch.int32), lp2.view(torch.int32))
        assert torch.equal(plp.view(torch.int32), plp2.view(torch.int32))
    print(f"V={V} {dtype} {ld_kind}: compared {kept}, left out {skipped}")
    # six rows per launch have something allowed; at most 5 % of all rows are left out
    assert kept + skipped == 6 * DRAWS and skipped <= 0.05 * 7 * DRAWS


@pytest.mark.parametrize("V,dtype,ld_kind", CASES, ids=IDS)
def test_temperature_zero_is_the_greedy_ops_bitwise(V, dtype, ld_kind):
    c = make_case(V, dtype, ld_kind, 0)
    zero = torch.zeros(c["B"])
    args, idx, lp, plp, state = _launch(c, V, temp=zero)
    st = c["state"].to(DEV)
    g_idx, g_lp, g_plp = ops.masked_argmax_timestamps(*args[:5], st, *args[6:11])
    assert torch.equal(idx, g_idx.cpu()) and torch.equal(state, st.cpu())
    assert torch.equal(lp.view(torch.int32), g_lp.cpu().view(torch.int32))
    assert torch.equal(plp.view(torch.int32), g_plp.cpu().view(torch.int32))
    assert not torch.equal(state, c["state"])
    # no ts_ctl: the probe op, with and without a temperature-0 key
    args, idx, lp, plp, state = _launch(c, V, temp=zero, ctl=None)
    p_idx, p_lp, p_plp = ops.masked_argmax_logprob_probe(*args[:4])
    assert torch.equal(idx, p_idx.cpu()) and torch.equal(state, c["state"])
    assert torch.equal(lp.view(torch.int32), p_lp.cpu().view(torch.int32))
    assert torch.equal(plp.view(torch.int32), p_plp.cpu().view(torch.int32))


@pytest.mark.parametrize("V", [520, 8232])
def test_rule_off_sampling_without_ts_ctl(V):
    """``ts_ctl`` absent: every row draws among its mask row's columns, the
    model's token under the device's noise; one chunk and two."""
    c = make_case(V, torch.float32, "pad64", 1)
    args, idx, lp, plp, state = _launch(c, V, ctl=None)
    assert torch.equal(state, c["state"])
    noise = ops.gumbel_noise(c["rng"].to(DEV), V).cpu()
    x = c["buf"][:c["B"], :V].float()
    w_idx, w_lp, _ = ref.masked_argmax_sample(x, c["mask"], c["rows"], c["probe"], None, None, None,
                                              0, 0, 0, 0, c["temp"], c["rng"], noise=noise)
    assert torch.equal(idx, w_idx) and int(idx[6]) == -1
    assert float((lp[:6] - w_lp[:6]).abs().max()) <= bound(V, torch.float32) + 2e-6


@pytest.mark.parametrize("Vn,T,seed", RULE_OFF, ids=[f"V{v}-T{t}" for v, t, _ in RULE_OFF])
def test_distribution_rule_off_on_the_device(Vn, T, seed):
    from scipy.stats import chi2
    x, temp, rng, p = dist_rule_off(Vn, T, seed)
    probe = torch.full((N_ROWS,), -1, dtype=torch.int32)
    idx, _, _ = ops.masked_argmax_sample(x.to(DEV), None, None, probe.to(DEV), None, None, None, 0,
                                         0, 0, 0, temp.to(DEV), rng.to(DEV))
    stat, df = chi_square(np.bincount(idx.cpu().numpy(), minlength=Vn).astype(np.float64), p)
    crit = float(chi2.isf(1e-6, df))
    print(f"V={Vn} T={T}: chi2 {stat:.1f} df {df} critical {crit:.1f}")
    assert stat < crit


@pytest.mark.parametrize("fires", [True, False], ids=["fires", "does-not-fire"])
def test_distribution_ruled_on_the_device(fires):
    from scipy.stats import chi2
    args, p = dist_ruled(fires, 11 + fires)
    dargs = [a.to(DEV) if torch.is_tensor(a) else a for a in args]
    idx = ops.masked_argmax_sample(*dargs)[0].cpu()
    assert bool((p[idx.numpy()] > 0).all())
    stat, df = chi_square(np.bincount(idx.numpy(), minlength=len(p)).astype(np.float64)[p > 0],
                          p[p > 0])
    crit = float(chi2.isf(1e-6, df))
    print(f"ruled, fires={fires}: chi2 {stat:.1f} df {df} critical {crit:.1f}")
    assert stat < crit
    word = int(args[5][0])
    assert dargs[5].cpu()[:-1].tolist() == [ref.ts_state_next(word, 2, int(i), TSB) for i in idx]

"""Temperature sampling in the row scan (``ops.masked_argmax_sample``; on the
CPU ``ops.reference.masked_argmax_sample``): the counter-based Gumbel noise,
the row key, the draw's distribution and its identity with the greedy ops at
temperature 0. The kernel is held to this reference, bit for bit in the index
and the state word, in ``tests/test_argmax_sample_gpu.py``, which also uses the
seven-row launches built here (``make_case``).

**Distribution.** 8192 rows of identical logits under the keys
``sample_key(s, 0, 1, i)``: Pearson's chi-square of the drawn columns against
``softmax(x / T)`` over the class Whisper would sample from (cells expecting
fewer than 5 draws are pooled), below ``chi2.isf(1e-6, df)``. The keys are
fixed, so the figure is too.

**Left-out rows.** The device's ``logf`` differs from the host's by a few ulp,
so a row whose two best keys lie within 4 f32 ulp of each other, or whose
mass-rule margin ``|d| < 1e-3`` (as in ``test_argmax_timestamps_gpu.py``), may
be decided either way there; ``test_left_out_budget`` checks with the
reference noise that such rows are at most 5 % of the sampled rows.
"""
import math

import numpy as np
import pytest
import torch
from test_argmax_logprob import R
from test_argmax_timestamps import EOT, MAXI, TSB, TSC, V, edge_cases
from test_argmax_timestamps_gpu import SHAPES, _ld, _states

from loqa_hub_amd import ops
from loqa_hub_amd.ops import reference as ref
from loqa_hub_amd.ops.reference import pack_mask

NINF = float("-inf")
MARGIN = 1e-3
KEY_ULPS = 4
N_ROWS = 8192
CASE_MAXI = 12          # max_initial of the seven-row launches (``make_case``)


# ------------------------------------------------------------------ noise, key
def test_uniform_is_exact_and_inside_the_unit_interval():
    u = ref.gumbel_uniform(torch.tensor([0, 0xFFFFFFFF, 1 << 9, 0x7FFFFFFF]))
    assert u.dtype == torch.float32
    assert u.tolist() == [2.0 ** -24, 1.0 - 2.0 ** -24, 3 * 2.0 ** -24, 0.5 - 2.0 ** -24]
    assert 0.0 < float(u.min()) and float(u.max()) < 1.0
    # every u is an odd multiple of 2^-24 below 2^24: exact in f32, and g is finite
    h = ref.gumbel_hash(torch.tensor([0, -1, 12345], dtype=torch.int32), 4096)
    assert int(h.min()) >= 0 and int(h.max()) < 1 << 32
    k = ref.gumbel_uniform(h).double() * 2.0 ** 24
    assert torch.equal(k, k.round()) and bool((k.long() % 2 == 1).all())
    g = ref.gumbel_noise(torch.tensor([0, -1, 12345], dtype=torch.int32), 4096)
    assert bool(torch.isfinite(g).all()) and -3.0 < float(g.min()) and float(g.max()) < 17.0
    lo = -math.log(-math.log(2.0 ** -24))
    hi = -math.log(-math.log1p(-2.0 ** -24))
    assert -2.9 < lo < -2.8 and 16.6 < hi < 16.7


def test_hash_matches_the_scalar_definition():
    rng = torch.tensor([7, -5], dtype=torch.int32)
    h = ref.gumbel_hash(rng, 40)
    for b, key in enumerate((7, (1 << 32) - 5)):
        for v in (0, 1, 39):
            assert int(h[b, v]) == ref.fmix32(key ^ ref.fmix32((v + 0x9E3779B9) & 0xFFFFFFFF))
    assert ref.fmix32(1) == int(ref._fmix32(torch.tensor([1]))[0])


def test_sample_key_separates_its_coordinates():
    base = ref.sample_key(3, 1, 2, 5)
    assert 0 <= base < 1 << 32 and base == ref.sample_key(3, 1, 2, 5)
    others = {ref.sample_key(4, 1, 2, 5), ref.sample_key(3, 0, 2, 5), ref.sample_key(3, 1, 1, 5),
              ref.sample_key(3, 1, 2, 6), ref.sample_key(3, 2, 1, 5), ref.sample_key(3, 5, 2, 1)}
    assert base not in others and len(others) == 6
    keys = {ref.sample_key(0, w, a, i) for w in range(4) for a in range(6) for i in range(96)}
    assert len(keys) == 4 * 6 * 96
    assert ref.key_i32(0xFFFFFFFF) == -1 and ref.key_i32(5) == 5
    assert ref.key_i32(1 << 31) == -(1 << 31)


# -------------------------------------------------------- temperature 0: greedy
def test_temperature_zero_is_the_timestamps_op():
    g = torch.Generator().manual_seed(4)
    B = 24
    x = torch.randn(B, V, generator=g) * 3
    x[:, TSB:] += 2.0
    bits = torch.rand(2, V, generator=g) < 0.6
    bits[:, EOT] = True
    mask = pack_mask(bits)
    rows = (torch.arange(B) % 2).to(torch.int32)
    probe = torch.where(torch.arange(B) % 3 == 0, 5, -1).to(torch.int32)
    ctl = (torch.arange(B) % 3).to(torch.int32)
    slot = torch.arange(B, dtype=torch.int32)
    words = [ref.ts_state_pack(7, False, True), ref.ts_state_pack(7, True, True),
             ref.ts_state_pack(7, True, False), ref.ts_state_pack(-1, False, False)]
    state = torch.tensor([words[b % 4] for b in range(B)] + [99], dtype=torch.int32)
    temp = torch.zeros(B)
    rng = torch.arange(B, dtype=torch.int32)
    for fn in (ref.masked_argmax_sample, ops.masked_argmax_sample):
        s1, s2 = state.clone(), state.clone()
        a = fn(x, mask, rows, probe, ctl, s1, slot, TSB, TSC, EOT, MAXI, temp, rng)
        b = ref.masked_argmax_timestamps(x, mask, rows, probe, ctl, s2, slot, TSB, TSC, EOT, MAXI)
        assert torch.equal(a[0], b[0]) and torch.equal(s1, s2) and not torch.equal(s1, state)
        for u, w in zip(a[1:], b[1:]):
            assert torch.equal(u.view(torch.int32), w.view(torch.int32))
        a = fn(x, mask, rows, probe, None, None, None, 0, 0, 0, 0, temp, rng)
        b = ref.masked_argmax_logprob_probe(x, mask, rows, probe)
        assert torch.equal(a[0], b[0])
        for u, w in zip(a[1:], b[1:]):
            assert torch.equal(u.view(torch.int32), w.view(torch.int32))


def test_decision_edges_survive_a_temperature():
    """The exact edge rows of ``test_argmax_timestamps.py`` whose winner's class
    holds one column (or nothing) give the same token, log-probability and
    state at any temperature: the mass rule is evaluated at temperature 1."""
    cases = [c for c in edge_cases() if c[0] in ("eot", "none")]
    B = len(cases)
    x = torch.stack([c[1] for c in cases])
    mask = pack_mask(torch.stack([c[2] for c in cases]))
    state = torch.tensor([c[3] for c in cases] + [4242], dtype=torch.int32)
    ctl = torch.tensor([c[4] for c in cases], dtype=torch.int32)
    slot = torch.arange(B, dtype=torch.int32)
    probe = torch.full((B,), -1, dtype=torch.int32)
    idx, lp, _ = ops.masked_argmax_sample(x, mask, None, probe, ctl, state, slot, TSB, TSC, EOT,
                                          MAXI, torch.full((B,), 0.8), slot.clone())
    for i, (name, _, _, word, _, want, want_lp, nxt) in enumerate(cases):
        assert int(idx[i]) == want and float(lp[i]) == float(np.float32(want_lp)), name
        assert int(state[i]) == (word if nxt is None else nxt), name
    # "two": the rule fires, so the draw is among the two timestamps only,
    # whatever the text logit's noise; the log-probability is -log 2 either way
    name, xr, mb, word, c, _, want_lp, _ = [c for c in edge_cases() if c[0] == "two"][0]
    n = 64
    st = torch.full((n,), word, dtype=torch.int32)
    idx, lp, _ = ops.masked_argmax_sample(
        xr[None].repeat(n, 1), pack_mask(mb[None]), torch.zeros(n, dtype=torch.int32),
        torch.full((n,), -1, dtype=torch.int32), torch.full((n,), 2, dtype=torch.int32), st,
        torch.arange(n, dtype=torch.int32), TSB, TSC, EOT, MAXI, torch.full((n,), 1.0),
        torch.arange(n, dtype=torch.int32))
    assert set(idx.tolist()) == {TSB + 3, TSB + 9}
    assert all(v == float(np.float32(want_lp)) for v in lp.tolist())
    assert st.tolist() == [ref.ts_state_pack(int(i) - TSB, True, False) for i in idx]


def test_minus_inf_winner_and_wrapper_checks():
    x = torch.full((2, V), NINF)
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)
    idx, lp, plp = ops.masked_argmax_sample(x, None, None, i32(-1, 3), None, None, None, 0, 0, 0, 0,
                                            torch.tensor([0.5, 1.0]), i32(1, 2))
    assert bool((idx >= 0).all()) and lp.tolist() == [NINF, NINF] and plp.tolist() == [0.0, NINF]
    x = torch.zeros(2, V)
    state = torch.zeros(3, dtype=torch.int32)
    for bad in (torch.tensor([0.5, -0.1]), torch.tensor([0.5, math.nan]),
                torch.tensor([math.inf, 0.0])):
        with pytest.raises(ValueError, match="temp"):
            ops.masked_argmax_sample(x, None, None, i32(-1, -1), i32(0, 0), state, i32(0, 1), TSB,
                                     TSC, EOT, MAXI, bad, i32(1, 2))
    with pytest.raises(AssertionError):
        ops.masked_argmax_sample(x, None, None, i32(-1, -1), i32(0, 0), state, i32(0, 1), TSB, TSC,
                                 EOT, MAXI, torch.zeros(2, dtype=torch.float64), i32(1, 2))
    with pytest.raises(AssertionError):
        ops.masked_argmax_sample(x, None, None, i32(-1, -1), i32(0, 0), state, i32(0, 1), TSB, TSC,
                                 EOT, MAXI, torch.zeros(2), torch.zeros(2, dtype=torch.int64))
    with pytest.raises(AssertionError, match="share a state slot"):
        ops.masked_argmax_sample(x, None, None, i32(-1, -1), i32(2, 2), state, i32(1, 1), TSB, TSC,
                                 EOT, MAXI, torch.zeros(2), i32(1, 2))
    with pytest.raises(ValueError, match="timestamp layout"):
        ops.masked_argmax_sample(x, None, None, i32(-1, -1), i32(0, 0), state, i32(0, 1), TSB,
                                 TSC + 1, EOT, MAXI, torch.zeros(2), i32(1, 2))


# ---------------------------------------------------------------- distribution
def chi_square(counts, p):
    """Pearson's statistic of ``counts`` against probabilities ``p`` (cells
    expecting fewer than 5 pooled into one) and its degrees of freedom."""
    n = counts.sum()
    e = p * n
    small = e < 5
    if small.any():
        counts = np.append(counts[~small], counts[small].sum())
        e = np.append(e[~small], e[small].sum())
    assert abs(e.sum() - n) < 1e-6 * n
    return float(((counts - e) ** 2 / e).sum()), len(e) - 1


def dist_keys(s):
    return torch.tensor([ref.key_i32(ref.sample_key(s, 0, 1, i)) for i in range(N_ROWS)],
                        dtype=torch.int32)


def dist_rule_off(Vn, T, seed):
    """(logits [N, V], temp, rng, expected probabilities [V]) of a rule-off case."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(Vn, generator=g) * 2
    p = torch.softmax(x.double() / T, dim=-1).numpy()
    return x[None].repeat(N_ROWS, 1).contiguous(), torch.full((N_ROWS,), T), dist_keys(seed), p


def dist_ruled(fires, seed, T=0.6):
    """A ruled row (text after text, timestamps from 8) whose mass rule fires /
    does not: (call arguments, expected probabilities over the V columns)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(V, generator=g) * 2
    x[TSB:] += 1.5 if fires else -3.0
    bits = torch.rand(V, generator=g) < 0.5
    bits[EOT] = True
    bits[EOT + 1:] = False
    word = ref.ts_state_pack(7, False, True)
    okx = bits.clone()
    okt = torch.zeros(V, dtype=torch.bool)
    okt[TSB + 8:TSB + TSC] = True
    x64 = x.double()
    lt = torch.logsumexp(x64.masked_fill(~okt, NINF), dim=-1)
    d = float(lt - x64.masked_fill(~okx, NINF).max())
    assert (d > 0) == fires and abs(d) > 0.1        # far from the rule's edge
    allowed = okt if fires else (okx | okt)
    p = torch.softmax((x64 / T).masked_fill(~allowed, NINF), dim=-1).numpy()
    n = N_ROWS
    args = (x[None].repeat(n, 1).contiguous(), pack_mask(bits[None]),
            torch.zeros(n, dtype=torch.int32), torch.full((n,), -1, dtype=torch.int32),
            torch.full((n,), 2, dtype=torch.int32), torch.full((n + 1,), word, dtype=torch.int32),
            torch.arange(n, dtype=torch.int32), TSB, TSC, EOT, MAXI, torch.full((n,), T),
            dist_keys(seed))
    return args, p


RULE_OFF = [(8, 1.0, 1), (8, 0.2, 2), (40, 0.6, 3)]


@pytest.mark.parametrize("Vn,T,seed", RULE_OFF, ids=[f"V{v}-T{t}" for v, t, _ in RULE_OFF])
def test_distribution_rule_off(Vn, T, seed):
    from scipy.stats import chi2
    x, temp, rng, p = dist_rule_off(Vn, T, seed)
    probe = torch.full((N_ROWS,), -1, dtype=torch.int32)
    idx, lp, _ = ops.masked_argmax_sample(x, None, None, probe, None, None, None, 0, 0, 0, 0,
                                          temp, rng)
    stat, df = chi_square(np.bincount(idx.numpy(), minlength=Vn).astype(np.float64), p)
    crit = float(chi2.isf(1e-6, df))
    print(f"V={Vn} T={T}: chi2 {stat:.1f} df {df} critical {crit:.1f}")
    assert stat < crit
    # the log-probability is the token's log-softmax at temperature 1
    want = torch.log_softmax(x[0].double(), dim=-1)[idx.long()]
    assert float((lp.double() - want).abs().max()) < 1e-5


@pytest.mark.parametrize("fires", [True, False], ids=["fires", "does-not-fire"])
def test_distribution_ruled(fires):
    from scipy.stats import chi2
    args, p = dist_ruled(fires, 11 + fires)
    state = args[5]
    idx, lp, _ = ops.masked_argmax_sample(*args)
    assert bool((p[idx.numpy()] > 0).all())            # only what the rules leave
    assert bool((idx >= TSB + 8).all()) if fires else bool((idx < TSB).any())
    stat, df = chi_square(np.bincount(idx.numpy(), minlength=V).astype(np.float64)[p > 0], p[p > 0])
    crit = float(chi2.isf(1e-6, df))
    print(f"ruled, fires={fires}: chi2 {stat:.1f} df {df} critical {crit:.1f}")
    assert stat < crit
    word = ref.ts_state_pack(7, False, True)
    assert state[:-1].tolist() == [ref.ts_state_next(word, 2, int(i), TSB) for i in idx]
    assert int(state[-1]) == word


# --------------------------------------------------- the seven-row launch cases
_CACHE: dict = {}
TEMPS = [0.0, 0.6, 0.2, 1.0, 0.8, 0.4, 0.6]


def make_case(Vn, dtype, ld_kind, draw=0):
    """CPU tensors of one launch of seven rows, built once per key: 0 a greedy
    ruled row (temp 0), 1 a sampled rule-off probing row, 2 a sampled ctl 1, 3
    a sampled lone timestamp, 4 a sampled closed pair, 5 a sampled
    text-after-text row, 6 a sampled row with nothing allowed (a closed pair
    under an empty mask row). The logits are the view [:B, :V] of a [B + 2, ld]
    buffer that is hostile everywhere else."""
    key = (Vn, dtype, ld_kind, draw)
    if key in _CACHE:
        return _CACHE[key]
    tsb, tsc, eot, shift = SHAPES[Vn]
    B = 7
    g = torch.Generator().manual_seed(13 * Vn + 100 * draw + (dtype == torch.bfloat16))
    ld = _ld(Vn, ld_kind)
    x = (torch.randn(B, Vn, generator=g) * 3).clamp_(-12, 12)
    x[:, tsb:tsb + tsc] += shift
    assert float(x.abs().max()) <= R
    x = x.to(dtype)
    bits = torch.zeros(3, Vn, dtype=torch.bool)
    bits[0, :eot] = torch.rand(eot, generator=g) < 0.5
    bits[0, eot] = True
    bits[1, torch.randint(Vn, (8,), generator=g)] = True     # row 2 of the table: nothing
    mask = pack_mask(bits)
    rows = torch.tensor([0, 1, 0, 0, 0, 0, 2], dtype=torch.int32)
    probe = torch.tensor([-1, 5, -1, -1, Vn - 1, -1, -1], dtype=torch.int32)
    ctl = torch.tensor([2, 0, 1, 2, 2, 2, 2], dtype=torch.int32)
    SENT = -77
    state = torch.full((12,), SENT, dtype=torch.int32)
    slot = torch.tensor([2, 11, 5, 4, 9, 7, 1], dtype=torch.int32)
    text, pair, lone, _ = _states(tsc)
    for s, w in ((2, text), (4, lone), (9, pair), (7, text), (1, pair)):
        state[s] = w
    temp = torch.tensor(TEMPS)
    rng = torch.tensor([ref.key_i32(ref.sample_key(Vn + draw, 0, 1, b)) for b in range(B)],
                       dtype=torch.int32)
    buf = torch.full((B + 2, ld), 40.0).to(dtype)
    buf[:B, :Vn] = x
    out = dict(buf=buf, bits=bits, mask=mask, rows=rows, probe=probe, ctl=ctl, state=state,
               slot=slot, temp=temp, rng=rng, B=B, sent=SENT, V=Vn)
    _CACHE[key] = out
    return out


def expect(c, noise):
    """The launch's expectation under ``noise`` (f32 [B, V]): per row (idx, fp64
    log-probability, next state word or None, left out), from
    ``ref.masked_argmax_sample(..., noise=noise)`` and the two left-out tests."""
    Vn, B = c["V"], c["B"]
    tsb, tsc, eot, _ = SHAPES[Vn]
    x = c["buf"][:B, :Vn].float()
    state = c["state"].clone()
    idx, lp, plp = ref.masked_argmax_sample(x, c["mask"], c["rows"], c["probe"], c["ctl"], state,
                                            c["slot"], tsb, tsc, eot, CASE_MAXI, c["temp"], c["rng"],
                                            noise=noise)
    key = (x.double() + c["temp"].double()[:, None] * noise.double()).float()
    x64 = x.double()
    out = []
    for b in range(B):
        ctl, T = int(c["ctl"][b]), float(c["temp"][b])
        okx = c["bits"][int(c["rows"][b])].clone()
        okt = torch.zeros(Vn, dtype=torch.bool)
        d = math.inf
        if ctl:
            word = int(c["state"][int(c["slot"][b])])
            text_ok, lo, hi = ref.ts_allowed(word, ctl, tsc, CASE_MAXI)
            okx[tsb:] = False
            okx[: (tsb, eot, 0)[text_ok]] = False
            okt[tsb + lo:tsb + hi + 1] = True
            if okx.any() and okt.any():
                d = float(torch.logsumexp(x64[b].masked_fill(~okt, NINF), dim=-1)
                          - x64[b].masked_fill(~okx, NINF).max())
        fire = bool(okt.any()) and (not okx.any() or d > 0)
        allowed = okt if fire else (okx | okt)
        skip = abs(d) < MARGIN
        i = int(idx[b])
        if i < 0:
            out.append((-1, NINF, None, False))
            continue
        if T > 0 and int(allowed.sum()) > 1:
            k = key[b][allowed].sort(descending=True).values[:2]
            skip = skip or float(k[0] - k[1]) <= KEY_ULPS * float(np.spacing(np.float32(abs(k[0]))))
        want_lp = float(x64[b, i] - torch.logsumexp(x64[b].masked_fill(~allowed, NINF), dim=-1))
        nxt = int(state[int(c["slot"][b])]) if ctl else None
        out.append((i, want_lp, nxt, skip))
    return out, plp


CASES = [(Vn, dt, ld) for Vn in (520, 8232) for dt in (torch.float32, torch.bfloat16)
         for ld in ("pad64", "odd")] + [(51866, torch.bfloat16, "pad64")]
IDS = [f"{v}-{'bf16' if dt == torch.bfloat16 else 'f32'}-{ld}" for v, dt, ld in CASES]
DRAWS = 4


def test_left_out_budget():
    """With the reference noise: the rows the two conditions leave out are at
    most 5 % of the sampled rows, every row class draws, and the cases of a
    launch are what ``make_case`` says they are."""
    n = out = 0
    for Vn, dt, ld in CASES:
        if ld == "odd":
            continue                        # the same logits as pad64
        tsb, tsc, eot, _ = SHAPES[Vn]
        for draw in range(DRAWS):
            c = make_case(Vn, dt, ld, draw)
            want, _ = expect(c, ref.gumbel_noise(c["rng"], Vn))
            assert want[6][0] == -1 and want[0][2] is not None
            assert tsb <= want[2][0] <= tsb + CASE_MAXI             # ctl 1: an initial timestamp
            assert want[3][0] >= eot                           # a lone timestamp: no text
            assert want[4][0] < tsb                            # a closed pair: no timestamp
            assert c["bits"][1, want[1][0]]                    # rule-off: the mask row's columns
            for b in range(1, 6):
                n += 1
                out += want[b][3]
    print(f"sampled rows {n}, left out {out}")
    assert n == 5 * DRAWS * 5 and out <= 0.05 * n


def test_key_gap_condition_on_the_distribution_rows():
    """The 8192-row trial: no row's two best keys lie within 4 ulp."""
    x, temp, rng, _ = dist_rule_off(40, 0.6, 3)
    key = (x.double() + 0.6 * ref.gumbel_noise(rng, 40).double()).float()
    k = key.sort(dim=1, descending=True).values
    gap = (k[:, 0] - k[:, 1]).numpy()
    assert int((gap <= KEY_ULPS * np.spacing(np.abs(k[:, 0].numpy()))).sum()) == 0

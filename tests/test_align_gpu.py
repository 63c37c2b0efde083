"""The four alignment kernels (``csrc/kernels/align.hip``) against the
definitions in ``ops/reference.py``: record and DTW bit for bit, scores and cost
within bounds derived here. u = 2^-24 (f32 unit roundoff).

**Scores bound.** Inputs are bf16, so every product q_i k_i is exact in f32.

* The MFMA sums D products (any order) into an f32 accumulator and one
  multiply applies the scale: ``ds <= (D + 1) u * scale * sum_i |q_i k_i|``,
  taken at the largest ``sum_i |q_i k_i|`` of the case (``S_abs``).
* The row maximum is an exact comparison; ``t = s - max`` rounds once:
  ``u |t| <= 2 u S_max`` with ``S_max = max |s|``.
* ``expf`` is accurate to 1 ulp (2u relative) and turns an argument error
  ``dt`` into a relative error ``dt``: each exponential is off by at most
  ``e_exp = 2 ds + 2 u S_max + 2u`` relative (both s and the maximum move by ds).
* The denominator sums F positive terms: ``ceil(F / 64)`` per lane, 6 butterfly
  steps: ``(ceil(F / 64) + 6) u`` relative; it also inherits ``e_exp``. The
  division rounds once more.

``|P - P_ref| <= P_ref * (2 e_exp + (ceil(F / 64) + 7) u)``, about 1.5e-4
relative at D = 64, N(0, 1) inputs. The fp64 model's own error (1e-16) is far
below u. Measured maximum of ``|P - P_ref| / bound``: 0.0054 (MI355X).
For F = 1 every P is exactly 1; the wrong-model check skips it.

**Cost bound.** Per (head, frame) column with values p_r, fp64 mean ``m``, std
``s``, ``Z = (p - m) / s``:

* the mean sums R values in order: ``|dm| <= R u m``; ``d = p - mean`` rounds
  once: every deviation is off by at most ``delta = u (R m + max |d|)``;
* the std is the RMS norm of the deviations, and a norm moves by at most the
  norm of the perturbation: ``|ds| <= delta``, plus ``(R / 2 + 3) u s`` for the
  sum of squares, the division by R and the square root;
* ``|dZ| <= delta / s + |Z| (delta / s + (R / 2 + 4) u)``, taken at the
  column's largest ``|Z|``.

The median of 7 moves by at most the largest error in its window, the mean
over A heads in order adds ``(A + 1) u max |Z|``. Columns whose rows are all
equal are exactly 0 on both sides. Measured maximum of ``|cost - model| /
bound``: 0.036 (MI355X).

**Hostile memory.** K rows at or beyond F, the other slots' K rows, the V
halves and every ``align_q`` position outside ``rows`` hold NaN or 1e30: any
read of them shows in P.
"""
import math

import numpy as np
import pytest
import torch

from loqa_hub_amd import ops
from loqa_hub_amd.ops import reference as ref
from test_align_reference import D, N_LEAD, PLANTED, _cost64, planted_case

U = 2.0 ** -24
H = 4                       # heads per layer in these cases
N_CTX, T_ENC = 448, 1500
HEADS = [(1, 2), (0, 1), (1, 0)]
gpu = pytest.mark.gpu
DEVICES = [pytest.param("cpu", id="cpu"), pytest.param("cuda", id="gpu", marks=gpu)]


# ----------------------------------------------------------------- cases
def scores_case(A: int, R: int, F: int, device="cpu", seed: int = 0):
    """(aq, rows, xkv, heads, k_row0, q [A, R, D], k [A, F, D]): one slot of a
    query store and two layers' K|V buffers (column blocks of one wider buffer,
    as the engine's ``xkv_all``) with hostile values around what may be read."""
    g = torch.Generator().manual_seed(seed * 7919 + 131 * R + F)
    heads = HEADS[:A]
    q = torch.randn(A, R, D, generator=g).to(torch.bfloat16)
    k = torch.randn(A, F, D, generator=g).to(torch.bfloat16)
    rows = torch.randperm(N_CTX, generator=g)[:R].to(torch.int32)
    aq = torch.full((A, N_CTX, D), float("nan"), dtype=torch.bfloat16)
    aq[:, 1::2] = 1e30
    aq[:, rows.long()] = q
    k_row0 = T_ENC                              # slot 1 of 2 (+ 8 rows behind it)
    buf = torch.full((2 * T_ENC + 8, 2 * 2 * H * D), float("nan"), dtype=torch.bfloat16)
    buf[::3] = 1e30
    xkv = [buf[:, i * 2 * H * D:(i + 1) * 2 * H * D] for i in range(2)]
    for a, (l, h) in enumerate(heads):
        xkv[l][k_row0:k_row0 + F, h * D:(h + 1) * D] = k[a]
    buf = buf.to(device)
    xkv = [buf[:, i * 2 * H * D:(i + 1) * 2 * H * D] for i in range(2)]
    return aq.to(device), rows.to(device), xkv, heads, k_row0, q, k


def scores_bound(q, k, F: int, scale: float) -> torch.Tensor:
    """The derived bound per element of P (fp64 [A, R, F])."""
    qa, ka = q.double().abs(), k.double().abs()
    s_abs = float(torch.einsum("ard,afd->arf", qa, ka).max())
    s_max = float((torch.einsum("ard,afd->arf", q.double(), k.double()) * scale).abs().max())
    ds = (D + 1) * U * scale * s_abs
    e_exp = 2 * ds + 2 * U * s_max + 2 * U
    rel = 2 * e_exp + (math.ceil(F / 64) + 7) * U
    return rel * ref.align_scores(q.double(), k.double(), scale) + 1e-38


def cost_bound(P64: np.ndarray, n_lead: int) -> np.ndarray:
    """The derived bound per element of the cost (fp64 [R - n_lead, F])."""
    A, R, F = P64.shape
    m = P64.mean(1, keepdims=True)
    d = P64 - m
    s = P64.std(1, keepdims=True)
    ok = s > 0
    Z = np.divide(d, s, out=np.zeros_like(d), where=ok)
    zmax = np.abs(Z).max(1, keepdims=True)
    delta = U * (R * m + np.abs(d).max(1, keepdims=True))
    rel = np.divide(delta, s, out=np.zeros_like(s), where=ok)
    tz = (rel * (1 + zmax) + zmax * (R / 2 + 4) * U)[:, 0]          # [A, F]
    if F > 3:
        tp = np.pad(tz, ((0, 0), (3, 3)), mode="reflect")
        tz = np.lib.stride_tricks.sliding_window_view(tp, 7, axis=-1).max(-1)
    return np.broadcast_to(tz.mean(0) + (A + 1) * U * zmax.max(), (R - n_lead, F))


# ------------------------------------------------------------ record
@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("Mpad", [16, 32])
def test_record_is_bitwise_and_writes_nothing_else(device, Mpad):
    g = torch.Generator().manual_seed(Mpad)
    lens = [1, 4, 2, 3] if Mpad == 16 else [3, 1, 4, 2, 4, 1, 2, 3]
    T, B, B_pad = sum(lens), len(lens), 8
    heads = [(1, 3), (0, 0), (1, 1)]
    qs = {l: torch.randn(Mpad, H * D, generator=g).to(torch.bfloat16) for l in (0, 1)}
    cu = np.zeros(B_pad + 1, np.int32)
    cu[1:B + 1] = np.cumsum(lens)
    cu[B + 1:] = T                                         # padding sequences are empty
    slots = np.full(Mpad, -1, np.int32)
    slots[:T] = np.arange(100, 100 + T)
    positions = np.zeros(Mpad, np.int32)
    start = [5, 0, 17, 444, 2, 9, 300, 40]
    for b, n in enumerate(lens):
        positions[cu[b]:cu[b] + n] = np.arange(start[b], start[b] + n)
    positions[T:] = 3                                      # padding rows: a live position
    row_slot = np.full(B_pad, 8, np.int32)                 # padding sequences: the trash slot
    row_slot[:B] = [6, 2, 7, 0, 5, 1, 3, 4][:B]            # out of order
    t = lambda a: torch.from_numpy(a).to(device)  # noqa: E731
    aq = torch.full((9, len(heads), N_CTX, D), float("nan"), dtype=torch.bfloat16)
    want = aq.clone()
    ref.align_record(qs, heads, positions, slots, cu, row_slot, want)
    assert int((~torch.isnan(want.float())).sum()) == T * len(heads) * D
    got = aq.clone().to(device)
    ops.align_record({l: q.to(device) for l, q in qs.items()}, heads, t(positions), t(slots), t(cu),
                     t(row_slot), got)
    assert torch.equal(got.cpu().view(torch.int16), want.view(torch.int16))
    # a slot or a position outside the store writes nothing
    row_slot[0], positions[cu[1]] = 9, N_CTX
    got2 = aq.clone().to(device)
    ops.align_record({l: q.to(device) for l, q in qs.items()}, heads, t(positions), t(slots), t(cu),
                     t(row_slot), got2)
    want2 = aq.clone()
    ref.align_record(qs, heads, positions, slots, cu, row_slot, want2)
    assert torch.equal(got2.cpu().view(torch.int16), want2.view(torch.int16))
    assert int((~torch.isnan(want2.float())).sum()) == (T - lens[0] - 1) * len(heads) * D


# ------------------------------------------------------------ scores
@gpu
@pytest.mark.parametrize("A", [1, 3])
@pytest.mark.parametrize("R", [4, 17, 33, 70])
@pytest.mark.parametrize("F", [1, 7, 64, 65, 750, 1500])
def test_scores_within_the_derived_bound(A, R, F):
    aq, rows, xkv, heads, k_row0, q, k = scores_case(A, R, F, "cuda")
    scale = 1.0 / math.sqrt(D)
    P = ops.align_scores(aq, rows, xkv, heads, k_row0, F).cpu()
    assert P.shape == (A, R, F) and P.dtype == torch.float32
    want = ref.align_scores(q.double(), k.double(), scale)
    ratio = ((P.double() - want).abs() / scores_bound(q, k, F, scale)).max()
    print(f"scores A={A} R={R} F={F}: max |err| / bound = {float(ratio):.4f}")
    assert torch.isfinite(P).all() and float(ratio) <= 1.0
    P2 = ops.align_scores(aq, rows, xkv, heads, k_row0, F).cpu()
    assert torch.equal(P, P2)


@pytest.mark.parametrize("R,F", [(4, 7), (17, 64), (70, 1500)])
def test_a_wrong_scores_model_misses_the_bound_100_fold(R, F):
    """K shifted by one frame, a wrong head and a missing scale each deviate
    from the fp64 model by >= 100 x the bound on these inputs (CPU)."""
    _, _, _, _, _, q, k = scores_case(3, R, F)
    scale = 1.0 / math.sqrt(D)
    want = ref.align_scores(q.double(), k.double(), scale)
    bound = scores_bound(q, k, F, scale)
    wrong = {"shifted": ref.align_scores(q.double(), k.double().roll(1, 1), scale),
             "head": ref.align_scores(q.double(), k.double().roll(1, 0), scale),
             "scale": ref.align_scores(q.double(), k.double(), 1.0)}
    for name, P in wrong.items():
        assert float(((P - want).abs() / bound).max()) >= 100.0, name
    # the CPU path of the op is the reference on the same bf16 inputs
    aq, rows, xkv, heads, k_row0, q, k = scores_case(3, R, F)
    P = ops.align_scores(aq, rows, xkv, heads, k_row0, F)
    assert torch.equal(P, ref.align_scores(q, k, scale))


# -------------------------------------------------------------- cost
@gpu
@pytest.mark.parametrize("A,R,F", [(1, 4, 1), (3, 5, 3), (3, 17, 4), (2, 33, 7), (3, 70, 65),
                                   (1, 20, 150), (3, 33, 750), (2, 70, 1500)])
def test_cost_within_the_derived_bound_on_the_gpus_own_scores(A, R, F):
    aq, rows, xkv, heads, k_row0, _, _ = scores_case(A, R, F, "cuda", seed=1)
    P = ops.align_scores(aq, rows, xkv, heads, k_row0, F)
    n_lead = min(N_LEAD, R - 1)
    c = ops.align_cost(P, n_lead)
    assert c.shape == (R - n_lead, F) and c.dtype == torch.float32
    P64 = P.cpu().double().numpy()
    ratio = (np.abs(c.cpu().double().numpy() - _cost64(P64, n_lead)) /
             (cost_bound(P64, n_lead) + 1e-300)).max()
    print(f"cost A={A} R={R} F={F}: max |err| / bound = {float(ratio):.4f}")
    assert torch.isfinite(c).all() and ratio <= 1.0
    assert torch.equal(c, ops.align_cost(P, n_lead))                # fixed order: bitwise
    buf = torch.full((R * F + 5,), float("nan"), device="cuda")
    c2 = ops.align_cost(P, n_lead, out=buf)
    assert torch.equal(c2, c) and torch.isnan(buf[(R - n_lead) * F:]).all()


# --------------------------------------------------------------- dtw
def _dtw_input(N: int, M: int, kind: str) -> torch.Tensor:
    g = torch.Generator().manual_seed(N * 2000 + M)
    if kind == "random":
        x = torch.randn(N, M, generator=g)
        x[N // 2] = 0.25                                   # ties: constant rows
        x[0] = 0.0
        x[:, M // 2] = -1.0
        return x
    # the GPU's own cost of random scores (A = 2 heads, 3 leading rows)
    P = torch.softmax(torch.randn(2, N + 3, M, generator=g) * 3, -1).cuda()
    return ops.align_cost(P, 3).cpu()


@gpu
@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 130, 448])
@pytest.mark.parametrize("M", [1, 2, 7, 64, 1500])
@pytest.mark.parametrize("kind", ["random", "cost"])
def test_dtw_is_the_reference_bit_for_bit(N, M, kind):
    x = _dtw_input(N, M, kind)
    want, total = ref.dtw(x, return_cost=True)
    tf, tot = ops.dtw(x.cuda())
    assert tf.dtype == torch.int32 and tf.shape == (N,)
    assert tf.cpu().tolist() == want.tolist()
    assert tot.cpu().numpy().tobytes() == np.float32(total).tobytes()


def test_wrapper_argument_checks():
    x = torch.zeros(3, 4)
    with pytest.raises(ValueError):
        ops.dtw(torch.zeros(449, 4))
    with pytest.raises(ValueError):
        ops.dtw(x.double())
    with pytest.raises(ValueError):
        ops.align_cost(torch.zeros(2, 3, 4), 3)
    with pytest.raises(ValueError):
        ops.align_cost(torch.zeros(33, 3, 4), 0)
    aq, rows, xkv, heads, k_row0, _, _ = scores_case(3, 4, 7)
    with pytest.raises(ValueError):
        ops.align_scores(aq, rows, xkv, heads[:2], k_row0, 7)
    with pytest.raises(ValueError):
        ops.align_scores(aq, rows, xkv, heads, k_row0, T_ENC + 9)
    with pytest.raises(ValueError):
        ops.align_scores(aq, rows.long(), xkv, heads, k_row0, 7)
    bad = rows.clone()
    bad[0] = N_CTX
    with pytest.raises(ValueError):
        ops.align_scores(aq, bad, xkv, heads, k_row0, 7)
    tf, tot = ops.dtw(x)                                    # the CPU path: the reference
    assert tf.tolist() == [0, 0, 0] and float(tot) == 0.0
    assert ops.dtw_workspace(448, 1500) == 1947 * 448


# ------------------------------------------------- the whole chain
@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("A,N,F", PLANTED)
def test_planted_alignment_through_the_chain(device, A, N, F):
    q, k, edges = planted_case(A, N, F)
    heads = HEADS[:A]
    R = N_LEAD + N
    rows = torch.arange(5, 5 + R, dtype=torch.int32)
    aq = torch.full((A, N_CTX, D), float("nan"), dtype=torch.bfloat16)
    aq[:, 5:5 + R] = q
    xkv = [torch.full((T_ENC, 2 * H * D), float("nan"), dtype=torch.bfloat16) for _ in range(2)]
    for a, (l, h) in enumerate(heads):
        xkv[l][:F, h * D:(h + 1) * D] = k[a]
    P = ops.align_scores(aq.to(device), rows.to(device), [x.to(device) for x in xkv], heads, 0, F)
    tf, _ = ops.dtw(ops.align_cost(P, N_LEAD))
    assert tf.cpu().tolist() == edges.tolist()

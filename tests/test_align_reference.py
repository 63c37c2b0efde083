"""The definitions of word-timestamp alignment in ``ops/reference.py`` on the
CPU: ``dtw`` against a brute-force minimum over all monotone paths,
``align_cost``'s edge cases, the alignment-head sources, and a planted
alignment recovered exactly through ``align_scores`` -> ``align_cost`` ->
``dtw``.

**Planted alignment.** Token i of N owns the frames of a band
``[edge_i, edge_{i+1})``, the edges distinct multiples of 8 frames, the first
at 0. Per head every token has a random +-1 vector of D = 64 entries; a frame's
K row is its band's vector plus 0.1 noise, a token's query is its vector, the
``N_LEAD`` leading rows are small noise, everything rounded to bf16. In-band
scores are 64 / 8 = 8, all others ~N(0, 1): the softmax puts a token's weight
on its band, the normalisation over rows and the median filter (width 7 < 8)
keep the band edges, and DTW must return exactly the planted edges.
"""
import numpy as np
import pytest
import torch

from loqa_hub_amd.ops import reference as ref

D = 64
N_LEAD = 3
PLANTED = [(1, 1, 8), (2, 5, 64), (3, 17, 200), (3, 40, 750), (2, 64, 1500)]


def planted_case(A: int, N: int, F: int, seed: int = 0):
    """(q [A, N_LEAD + N, D] bf16, k [A, F, D] bf16, edges int [N])."""
    g = np.random.default_rng(1000 * seed + 7 * N + F)
    edges = np.sort(np.concatenate([[0], 8 * (1 + g.choice(F // 8 - 1, N - 1, replace=False))])) \
        if N > 1 else np.zeros(1, np.int64)
    band = np.searchsorted(edges, np.arange(F), side="right") - 1
    v = g.choice([-1.0, 1.0], size=(A, N, D))
    k = v[:, band] + 0.1 * g.standard_normal((A, F, D))
    q = np.concatenate([0.05 * g.standard_normal((A, N_LEAD, D)), v], axis=1)
    to = lambda x: torch.from_numpy(x).to(torch.bfloat16)  # noqa: E731
    return to(q), to(k), edges.astype(np.int64)


def brute_force(x: np.ndarray):
    """Minimum cost over all monotone paths (0, 0) -> (N - 1, M - 1) with steps
    (1, 1), (1, 0), (0, 1), in fp64; (cost, first column of every row)."""
    N, M = x.shape
    best = (np.inf, None)

    def walk(i, j, cost, first):
        nonlocal best
        cost += x[i, j]
        if i == N - 1 and j == M - 1:
            if cost < best[0]:
                best = (cost, list(first))
            return
        for di, dj in ((1, 1), (1, 0), (0, 1)):
            a, b = i + di, j + dj
            if a < N and b < M:
                walk(a, b, cost, first + [b] if di else first)
    walk(0, 0, 0.0, [0])
    return best


@pytest.mark.parametrize("N,M", [(n, m) for n in range(1, 6) for m in range(1, 6)])
def test_dtw_is_the_brute_force_minimum(N, M):
    g = np.random.default_rng(10 * N + M)
    # distinct multiples of 1/64 below 2^6: every path sum is exact in f32 and in
    # fp64; these fixed draws leave no two best paths tied (a tie would show as a
    # mismatch of the first columns)
    x = (g.permutation(4096)[: N * M].reshape(N, M) / 64.0).astype(np.float32)
    cost, first = brute_force(x.astype(np.float64))
    tf, total = ref.dtw(x, return_cost=True)
    assert float(total) == cost
    assert tf.dtype == np.int32 and tf.tolist() == first


@pytest.mark.parametrize("N,M", [(1, 1), (1, 9), (7, 1), (9, 4), (33, 5)])
def test_dtw_degenerate_shapes(N, M):
    g = np.random.default_rng(N * 100 + M)
    x = g.standard_normal((N, M)).astype(np.float32)
    tf, total = ref.dtw(x, return_cost=True)
    assert tf.shape == (N,) and tf[0] == 0
    assert np.all(np.diff(tf) >= 0) and 0 <= tf.min() and tf.max() < M
    if M == 1:
        assert tf.tolist() == [0] * N                      # the path goes vertical
        assert total == np.cumsum(x[:, 0], dtype=np.float32)[-1]
    if N == 1:
        assert total == np.cumsum(x[0], dtype=np.float32)[-1]
    if N > M:
        assert len(set(tf.tolist())) <= M                  # rows share frames


def test_dtw_wavefront_is_the_literal_recurrence():
    g = np.random.default_rng(3)
    for N, M in [(1, 1), (2, 7), (13, 29), (40, 17), (64, 65)]:
        x = g.standard_normal((N, M)).astype(np.float32)
        x[N // 2] = 0.25                                   # ties: a constant row
        x[:, M // 3] = x[0, M // 3]
        a, ca = ref.dtw(x, return_cost=True)
        b, cb = ref.dtw(x, return_cost=True, literal=True)
        assert a.tolist() == b.tolist() and ca.tobytes() == cb.tobytes()
    assert ref.dtw(torch.zeros(3, 5)).tolist() == ref.dtw(np.zeros((3, 5)), literal=True).tolist()


def _cost64(P, n_lead):
    """fp64 model of ``align_cost`` written independently (numpy)."""
    P = np.asarray(P, np.float64)
    mean = P.mean(1, keepdims=True)
    std = P.std(1, keepdims=True)
    Z = np.divide(P - mean, std, out=np.zeros_like(P), where=std != 0)
    if Z.shape[-1] > 3:
        Zp = np.pad(Z, ((0, 0), (0, 0), (3, 3)), mode="reflect")
        Z = np.median(np.lib.stride_tricks.sliding_window_view(Zp, 7, axis=-1), axis=-1)
    return -Z.mean(0)[n_lead:]


@pytest.mark.parametrize("F", [1, 3, 4, 7, 8, 33])
def test_cost_matches_the_numpy_model(F):
    g = torch.Generator().manual_seed(F)
    P = torch.softmax(torch.randn(3, 9, F, generator=g, dtype=torch.float64) * 2, -1)
    c = ref.align_cost(P, 2)
    assert c.shape == (7, F) and c.dtype == torch.float64
    np.testing.assert_allclose(c.numpy(), _cost64(P.numpy(), 2), rtol=0, atol=1e-12)
    assert ref.align_cost(P.float(), 2).dtype == torch.float32


def test_cost_edge_cases():
    g = torch.Generator().manual_seed(1)
    for F in (1, 3):        # no filter: the normalised value itself
        P = torch.rand(2, 6, F, generator=g, dtype=torch.float64)
        Z = (P - P.mean(1, keepdim=True)) / P.std(1, unbiased=False, keepdim=True)
        assert torch.allclose(ref.align_cost(P, 1), -Z.mean(0)[1:], atol=1e-12, rtol=0)
    # F = 4: reflect padding, frame 0's window is frames 3 2 1 0 1 2 3
    P = torch.rand(1, 5, 4, generator=g, dtype=torch.float64)
    Z = ((P - P.mean(1, keepdim=True)) / P.std(1, unbiased=False, keepdim=True))[0]
    want0 = torch.stack([Z[:, i] for i in (3, 2, 1, 0, 1, 2, 3)], -1).median(-1).values
    want3 = torch.stack([Z[:, i] for i in (0, 1, 2, 3, 2, 1, 0)], -1).median(-1).values
    c = ref.align_cost(P, 0)
    assert torch.allclose(c[:, 0], -want0, atol=1e-12) and torch.allclose(c[:, 3], -want3, atol=1e-12)
    # a frame with equal scores in every row normalises to 0 (std == 0), not NaN
    P = torch.rand(2, 4, 9, generator=g)
    P[:, :, 4] = 0.125
    P[:, :, :3] = 0.5
    c = ref.align_cost(P, 0)
    assert torch.isfinite(c).all() and (c[:, 0] == 0).all()


def test_scores_are_the_scaled_softmax():
    g = torch.Generator().manual_seed(0)
    q = torch.randn(2, 5, D, generator=g).to(torch.bfloat16)
    k = torch.randn(2, 11, D, generator=g).to(torch.bfloat16)
    P = ref.align_scores(q, k, 0.125)
    assert P.shape == (2, 5, 11) and P.dtype == torch.float32
    s = (q[1, 3].double() * k[1].double()).sum(-1) * 0.125
    assert torch.allclose(P[1, 3].double(), torch.softmax(s, 0), atol=1e-6)
    assert ref.align_scores(q.double(), k.double(), 0.125).dtype == torch.float64
    assert ref.align_frames(1, 1500) == 1 and ref.align_frames(0, 1500) == 1
    assert ref.align_frames(321, 1500) == 2 and ref.align_frames(48000, 1500) == 150
    assert ref.align_frames(480000, 1500) == 1500 and ref.align_frames(10 ** 7, 1500) == 1500


def test_alignment_head_sources():
    h = ref.alignment_heads
    assert h(4, 2) == [(2, 0), (2, 1), (3, 0), (3, 1)]               # the upper half
    assert h(4, 2, None, {"alignment_heads": [[1, 0], [3, 1]]}) == [(1, 0), (3, 1)]
    assert h(4, 2, " 0:1, 3:0 ", {"alignment_heads": [[1, 0]]}) == [(0, 1), (3, 0)]
    assert h(4, 2, "", {}) == h(4, 2)
    with pytest.raises(ValueError, match="HUB_STT_ALIGNMENT_HEADS"):
        h(32, 20)                                                    # 320 heads by default
    with pytest.raises(ValueError, match="HUB_STT_ALIGNMENT_HEADS"):
        h(4, 2, ",".join(f"{i % 4}:{i % 2}" for i in range(33)))
    for bad in ("1", "1:x", "4:0", "0:2", "1:0,1:0", "-1:0"):
        with pytest.raises(ValueError, match="HUB_STT_ALIGNMENT_HEADS"):
            h(4, 2, bad)
    assert len(h(32, 20, ",".join(f"{l}:{l % 20}" for l in range(32)))) == 32


@pytest.mark.parametrize("A,N,F", PLANTED)
@pytest.mark.parametrize("dt", [torch.float32, torch.float64])
def test_planted_alignment_is_recovered(A, N, F, dt):
    for seed in range(2):
        q, k, edges = planted_case(A, N, F, seed)
        P = ref.align_scores(q.to(dt), k.to(dt), 1.0 / np.sqrt(D))
        cost = ref.align_cost(P, N_LEAD)
        assert cost.shape == (N, F)
        assert ref.dtw(cost.float()).tolist() == edges.tolist()


def test_align_record_reference():
    H, T = 2, 6
    qs = {1: torch.arange(T * H * D, dtype=torch.float32).view(T, H * D).to(torch.bfloat16)}
    aq = torch.full((3, 2, 8, D), float("nan"), dtype=torch.bfloat16)
    positions = torch.tensor([0, 1, 2, 5, 0, 0], dtype=torch.int32)
    slots = torch.tensor([4, 5, 6, 9, -1, -1], dtype=torch.int32)
    cu_q = torch.tensor([0, 3, 4, 4], dtype=torch.int32)
    row_slot = torch.tensor([2, 0, 1], dtype=torch.int32)
    ref.align_record(qs, [(1, 1), (1, 0)], positions, slots, cu_q, row_slot, aq)
    want = torch.full_like(aq, float("nan"))
    for r, (s, p) in enumerate([(2, 0), (2, 1), (2, 2), (0, 5)]):
        want[s, 0, p] = qs[1][r, D:]
        want[s, 1, p] = qs[1][r, :D]
    assert torch.equal(aq.view(torch.int16), want.view(torch.int16))

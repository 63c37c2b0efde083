"""The host definitions of beam search (``ops.reference``): ``beam_topk``,
``beam_merge``, ``BeamState`` / ``beam_search``.

``beam_search`` is held to a literal transcription of openai/whisper's
``BeamSearchDecoder.update`` / ``finalize`` and ``MaximumLikelihoodRanker``
(patience 1, no length penalty) written here: a dict of scores keyed by the
extended prefix, ``topk(B + 1)`` per beam, a walk over the sorted dict, the
fill from the live beams, the rank by sum / length. The toy models are tables
of integer logits (V = 12) keyed by a hash of the prefix, drawn so that no two
candidate scores of a step tie; token lists, sums and the winner must agree.
"""
import math

import numpy as np
import pytest
import torch

from loqa_hub_amd.ops import reference as ref
from loqa_hub_amd.ops.reference import pack_mask

V, EOT, MAX_NEW = 12, 3, 6


def toy_model(seed: int):
    """prefix -> integer logits row [V]; EOT grows likelier with the length."""
    rows: dict = {}

    def step(prefix):
        key = tuple(prefix)
        if key not in rows:
            g = torch.Generator().manual_seed(seed * 7919 + hash(key) % 100003)
            # distinct integers of a wider range: rows differ in their sums too
            # (even; EOT odd, so that it never equals another logit of its row)
            x = torch.randperm(2 * V, generator=g)[:V].float() * 2
            x[EOT] = x[EOT] - 11 + 6 * len(key)
            rows[key] = x
        return rows[key]
    return step


def whisper_literal(step, B: int, eot: int, max_new: int):
    """openai/whisper decoding.py, transcribed for one audio."""
    beams = [()]                      # token prefixes after sample_begin
    sums = [0.0]
    finished: dict = {}
    for _ in range(max_new):
        logprobs = [torch.log_softmax(step(list(p)).float(), dim=-1) for p in beams]
        scores, sources = {}, {}
        for idx, prefix in enumerate(beams):
            vals, toks = logprobs[idx].topk(min(B + 1, V))
            for lp, t in zip(vals.tolist(), toks.tolist()):
                # the f32 accumulation of the kernels: one rounding per step
                scores[prefix + (t,)] = float(np.float32(np.float32(sums[idx]) + np.float32(lp)))
                sources[prefix + (t,)] = idx
        assert len(set(scores.values())) == len(scores), "the toy model ties"
        saved = 0
        new_beams, new_sums, newly = [], [], {}
        for seq in sorted(scores, key=scores.get, reverse=True):
            if seq[-1] == eot:
                newly[seq] = scores[seq]
            else:
                new_beams.append(seq)
                new_sums.append(scores[seq])
                saved += 1
                if saved == B:
                    break
        beams, sums = new_beams, new_sums
        for seq in sorted(newly, key=newly.get, reverse=True):
            if len(finished) >= B:
                break
            finished[seq] = newly[seq]
        if len(finished) >= B:
            break
    if len(finished) < B:             # finalize: fill up from the live beams
        for i in np.argsort(sums)[::-1]:
            finished[beams[i] + (eot,)] = sums[i]
            if len(finished) >= B:
                break
    seqs = list(finished)
    lengths = [len([t for t in s if t != eot]) for s in seqs]
    winner = int(np.argmax([finished[s] / max(1, n) for s, n in zip(seqs, lengths)]))
    return [(list(s), finished[s]) for s in seqs], winner


@pytest.mark.parametrize("B", [1, 2, 3, 5])
@pytest.mark.parametrize("seed", [0, 1, 2, 3, 5, 6])   # seeds whose tables never tie
def test_beam_search_is_whispers(seed, B):
    step = toy_model(seed)
    hyps, winner = ref.beam_search(step, B, EOT, MAX_NEW)
    want, want_winner = whisper_literal(step, B, EOT, MAX_NEW)
    assert len(hyps) == len(want) == B
    strip = lambda t: [x for x in t if x != EOT]
    for (t, s, lps), (wt, ws) in zip(hyps, want):
        # Whisper appends EOT to a live beam it fills up with; here the tokens
        # of such a hypothesis end where the beam does
        assert strip(t) == strip(wt)
        assert s == pytest.approx(ws, abs=1e-4)
        assert len(lps) == len(t)
        assert sum(lps) == pytest.approx(s, abs=1e-4)
    assert winner == want_winner


@pytest.mark.parametrize("seed", range(4))
def test_beam_one_is_greedy(seed):
    step = toy_model(seed)
    (tokens, s, lps), = ref.beam_search(step, 1, EOT, MAX_NEW)[0]
    greedy, total = [], 0.0
    while len(greedy) < MAX_NEW:
        lp = torch.log_softmax(step(greedy), dim=-1)
        t = int(lp.argmax())
        greedy.append(t)
        total += float(lp[t])
        if t == EOT:
            break
    assert tokens == greedy
    assert s == pytest.approx(total, abs=1e-4)


def _row(vals):
    return torch.tensor([vals], dtype=torch.float32)


def test_topk_fewer_allowed_than_kb():
    x = _row([1, 5, 3, 0, 2, 4])
    allowed = torch.tensor([[True, False, True, True, False, False]])
    cid, clp, elp = ref.beam_topk(x, pack_mask(allowed), None, eot=3, KB=4)
    assert cid.tolist() == [[2, 0, -1, -1]]
    lse = math.log(math.exp(1) + math.exp(3) + math.exp(0))
    assert clp[0, :2].tolist() == pytest.approx([3 - lse, 1 - lse], abs=1e-6)
    assert clp[0, 2:].tolist() == [float("-inf")] * 2
    assert elp.item() == pytest.approx(0 - lse, abs=1e-6)


def test_topk_fully_masked_row():
    x = _row([1, 5, 3, 0])
    cid, clp, elp = ref.beam_topk(x, pack_mask(torch.zeros(1, 4, dtype=torch.bool)), None, 3, 2)
    assert cid.tolist() == [[-1, -1]]
    assert clp.tolist() == [[float("-inf")] * 2] and elp.tolist() == [float("-inf")]
    out = ref.beam_merge(cid, clp, elp, torch.tensor([[0.0, float("-inf")]]), 1)
    tok, parent, lp, cum, es, fin = (o[0].tolist() for o in out)
    assert tok == [-1, -1] and parent == [-1, -1]
    assert lp == cum == [float("-inf")] * 2
    assert es == [float("-inf")] * 2
    assert fin == [1, 0]              # fewer than B candidates; the host ignores a -inf score


def test_topk_eot_is_the_row_maximum_and_never_a_candidate():
    x = _row([1, 5, 3, 9, 2])
    cid, clp, elp = ref.beam_topk(x, None, None, eot=3, KB=3)
    assert cid.tolist() == [[1, 2, 4]]
    lse = torch.logsumexp(x[0], 0).item()
    assert elp.item() == pytest.approx(9 - lse, abs=1e-6)
    assert clp[0].tolist() == pytest.approx([5 - lse, 3 - lse, 2 - lse], abs=1e-6)
    # n_src = 1: EOT scores above the B-th extension -> it finishes
    out = ref.beam_merge(cid, clp, elp, torch.tensor([[0.0, -1.0, -2.0]]), 1)
    tok, parent, lp, cum, es, fin = (o[0].tolist() for o in out)
    assert tok == [1, 2, 4] and parent == [0, 0, 0] and fin == [1, 0, 0]
    assert es[1:] == [float("-inf")] * 2


def test_topk_eot_masked():
    x = _row([1, 5, 3, 9, 2])
    allowed = torch.tensor([[True, True, True, False, True]])
    cid, clp, elp = ref.beam_topk(x, pack_mask(allowed), None, eot=3, KB=2)
    assert cid.tolist() == [[1, 2]] and elp.tolist() == [float("-inf")]
    lse = math.log(sum(math.exp(v) for v in (1, 5, 3, 2)))     # EOT is out of the sum
    assert clp[0].tolist() == pytest.approx([5 - lse, 3 - lse], abs=1e-6)
    out = ref.beam_merge(cid, clp, elp, torch.tensor([[0.0, 0.0]]), 1)
    assert out[5][0].tolist() == [0, 0]


def test_ties_score_then_source_beam_then_column():
    # two source beams with equal sums and equal rows: every score ties
    x = torch.tensor([[2.0, 7, 7, 0, 7], [2.0, 7, 7, 0, 7]])
    cid, clp, elp = ref.beam_topk(x, None, None, eot=3, KB=2)
    assert cid.tolist() == [[1, 2], [1, 2]]                     # equal logits: lower column
    out = ref.beam_merge(cid, clp, elp, torch.tensor([[-1.0, -1.0]]), 2)
    tok, parent = out[0][0].tolist(), out[1][0].tolist()
    assert (tok, parent) == ([1, 2], [0, 0])                    # lower source beam first
    # a better sum moves beam 1 in front
    out = ref.beam_merge(cid, clp, elp, torch.tensor([[-1.0, -0.5]]), 2)
    assert (out[0][0].tolist(), out[1][0].tolist()) == ([1, 2], [1, 1])
    # equal scores across beams from different columns: beam first, then column
    cid = torch.tensor([[4, 2], [1, 3]], dtype=torch.int32)
    clp = torch.tensor([[-1.0, -1.0], [-1.0, -1.0]])
    out = ref.beam_merge(cid, clp, torch.tensor([-9.0, -9.0]), torch.tensor([[0.0, 0.0]]), 2)
    assert (out[0][0].tolist(), out[1][0].tolist()) == ([2, 4], [0, 0])


def test_merge_strictly_above_and_minus_inf_inputs():
    cid = torch.tensor([[1, 2], [4, 5]], dtype=torch.int32)
    clp = torch.tensor([[-1.0, -2.0], [-1.0, -3.0]])
    # beam 0's EOT ties the B-th selected score (-2): not strictly above, not finished
    elp = torch.tensor([-2.0, float("-inf")])
    out = ref.beam_merge(cid, clp, elp, torch.tensor([[0.0, -1.0]]), 2)
    tok, parent, lp, cum, es, fin = (o[0].tolist() for o in out)
    assert tok == [1, 2] and parent == [0, 0] and cum == [-1.0, -2.0]
    assert es == [-2.0, float("-inf")] and fin == [0, 0]
    # a dead source beam (-inf sum) never wins and never finishes
    out = ref.beam_merge(cid, clp, torch.tensor([-0.5, -0.5]),
                         torch.tensor([[0.0, float("-inf")]]), 2)
    tok, parent, lp, cum, es, fin = (o[0].tolist() for o in out)
    assert parent == [0, 0] and fin == [1, 0] and es[1] == float("-inf")


def test_copy_pairs_are_checked():
    assert ref.check_copy_pairs([(0, 1), (0, 2)], 4).tolist() == [[0, 1], [0, 2]]
    for bad in ([(0, 1), (1, 2)], [(0, 2), (1, 2)], [(0, 4)], [(-1, 2)], [(1, 1)]):
        with pytest.raises(ValueError):
            ref.check_copy_pairs(bad, 4)

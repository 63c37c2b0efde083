"""The start-of-transcript probe with a checkpoint's own tokenizer
(``HFTokenizer``): the candidate languages and the no-speech token come from
the file (or its generation config), and the mask table's row 0 is the
checkpoint's suppress mask. Byte-level BPE trained here, as in
``tests/test_tokenizer_hf.py``; CPU engine, ``test-whisper``."""
import json
import os

import numpy as np
import pytest
import torch

from loqa_hub_amd.engine.stt_engine import STTEngine, STTRequest
from loqa_hub_amd.engine.tokenizer import load_tokenizer
from loqa_hub_amd.models.configs import whisper_config
from loqa_hub_amd.ops.reference import unpack_mask

tk = pytest.importorskip("tokenizers")

CORPUS = ["turn on the kitchen lights and play music in the bedroom",
          "turn off the tv then dim the living room lamp", "hello what time is it"] * 20
# Whisper's order: the language tokens sit between SOT and <|translate|>
SPECIALS = ["<|endoftext|>", "<|startoftranscript|>", "<|en|>", "<|de|>", "<|fr|>", "<|haw|>",
            "<|translate|>", "<|transcribe|>", "<|startoflm|>", "<|startofprev|>", "<|nospeech|>",
            "<|notimestamps|>", "<|0.00|>"]


def _tokenizer(path, specials):
    from tokenizers import Tokenizer, decoders, models, pre_tokenizers, trainers
    t = Tokenizer(models.BPE())
    t.pre_tokenizer = pre_tokenizers.ByteLevel(add_prefix_space=False)
    t.decoder = decoders.ByteLevel()
    t.train_from_iterator(CORPUS, trainers.BpeTrainer(
        vocab_size=600, special_tokens=list(specials),
        initial_alphabet=pre_tokenizers.ByteLevel.alphabet()))
    os.makedirs(path, exist_ok=True)
    t.save(os.path.join(path, "tokenizer.json"))
    return os.path.join(path, "tokenizer.json")


def _engine(tok, **kw):
    return STTEngine(whisper_config("test-whisper"), torch.device("cpu"), seed=0, max_batch=2,
                     tokenizer=tok, **kw)


def test_languages_from_the_added_tokens(tmp_path):
    tok = load_tokenizer(_tokenizer(str(tmp_path / "w"), SPECIALS), 4096)
    ids = {c: tok.token_id(f"<|{c}|>") for c in ("en", "de", "fr", "haw")}
    assert tok.language_tokens() == ids and list(ids.values()) == [2, 3, 4, 5]
    eng = _engine(tok, language="auto")
    assert eng.tok is tok and eng.nospeech == tok.token_id("<|nospeech|>") == 10
    assert eng.lang_codes == ["en", "de", "fr", "haw"] and eng.lang_ids == [2, 3, 4, 5]
    # the mask table: row 0 = today's suppress mask, row 1 = the candidates
    rows = unpack_mask(eng._sup.cpu(), 4096)
    assert rows.shape == (2, 4096)
    assert torch.equal(rows[0], tok.sampling_mask(keep=(eng.eot,)))
    assert rows[1].nonzero()[:, 0].tolist() == [2, 3, 4, 5]
    sub = _engine(tok, language="auto", languages=["fr", "en"], weights=eng.weights)
    assert sub.lang_codes == ["en", "fr"]
    assert unpack_mask(sub._sup.cpu(), 4096)[1].nonzero()[:, 0].tolist() == [2, 4]
    fixed = _engine(tok, language="de", no_speech=True, weights=eng.weights)
    assert fixed.lang_codes == ["de"] and fixed.sot[1] == 3
    assert unpack_mask(fixed._sup.cpu(), 4096)[1].nonzero()[:, 0].tolist() == [3]
    for kw in ({"language": "auto", "languages": ["es"]}, {"language": "es", "sot_probe": True}):
        with pytest.raises(ValueError, match="language"):
            _engine(tok, weights=eng.weights, **kw)
    # free decoding: the language is a candidate, the text tokens are not special
    rng = np.random.default_rng(1)
    r = STTRequest((rng.standard_normal(16000) * 3000).astype(np.int16), max_new_tokens=5)
    sub.transcribe([r])
    assert r.language in ("en", "fr") and 0.5 <= r.language_prob < 1.0
    assert r.chunks[-1] == [r.lang_id, tok.token_id("<|transcribe|>"),
                            tok.token_id("<|notimestamps|>")]
    assert 0.0 < r.no_speech_prob < 1.0 and len(r.tokens) > 0
    assert all(t == eng.eot or t >= len(SPECIALS) for t in r.tokens)


def test_languages_from_the_generation_config_and_nocaptions(tmp_path):
    old = [s if s != "<|nospeech|>" else "<|nocaptions|>" for s in SPECIALS]
    f = _tokenizer(str(tmp_path / "w"), old)
    with open(os.path.join(os.path.dirname(f), "generation_config.json"), "w") as fh:
        json.dump({"lang_to_id": {"<|fr|>": 4, "<|en|>": 2}, "suppress_tokens": [20]}, fh)
    tok = load_tokenizer(f, 4096)
    assert tok.language_tokens() == {"en": 2, "fr": 4}
    assert list(tok.language_tokens()) == ["en", "fr"]
    eng = _engine(tok, language="")
    assert eng.auto_language and eng.lang_codes == ["en", "fr"]
    assert eng.nospeech == tok.token_id("<|nocaptions|>") == 10
    with pytest.raises(ValueError, match="language"):
        _engine(tok, language="auto", languages=["de"], weights=eng.weights)


def test_no_no_speech_token_is_an_error(tmp_path):
    few = [s for s in SPECIALS if s != "<|nospeech|>"]
    tok = load_tokenizer(_tokenizer(str(tmp_path / "w"), few), 4096)
    _engine(tok)                                   # fine without the probe
    with pytest.raises(ValueError, match="nospeech"):
        _engine(tok, no_speech=True)

"""Batched on-GPU speech-to-text (Whisper) - replaces the reference's external
OpenAI-compatible STT round trip (``stt_client.go:207-362``: float32->WAV encode,
multipart POST, JSON decode) with: pinned PCM16 -> H2D -> fused convert+RMS
kernel -> log-mel -> encoder -> greedy decoder, batched across utterances.

Random-init weights cannot produce a real transcript, so benchmark/synthetic
requests carry their known transcript and the decoder is *teacher-forced* to it
(SURVEY §7.4 item 1): every step still runs the full decoder forward and the
argmax over the 51 866-entry vocabulary, so cost is that of a real greedy decode
of the same length; only the fed-back token is the reference one.
"""
from __future__ import annotations

import collections
import logging
import os
import queue
import threading
import time
import weakref
import zlib
from concurrent.futures import FIRST_COMPLETED, Future, ThreadPoolExecutor, wait
from dataclasses import dataclass, field

import numpy as np
import torch

from .. import ops
from ..models.configs import WhisperConfig
from ..models.whisper import WhisperModel, WhisperWeights, decode_step_fast, decode_step_fused
from ..utils.tracing import tracer
from .batching import join_futures, plan_step
from .kv_cache import PagedKVCache
from .step_io import StepIO, StepLayout, decode_buckets, fill_meta, step_shapes, to_device
from .stt_segments import cut_window, text_tokens, utterance_segments
from .stt_words import utterance_words, window_words
from .tokenizer import (SyntheticTimestampTokenizer, SyntheticTokenizer, SyntheticWhisperTokenizer,
                        get_tokenizer)

log = logging.getLogger("loqa.stt")

N_SAMPLES = 480000  # 30 s @ 16 kHz
# numpy PCM of direct submissions staged through the pinned stager (False: a
# one-off pinned tensor copy per request)
PCM_STAGER = True
# relay PCM copied to HBM chunk by chunk while the relay speaks (pcm_staging.py)
PCM_STREAM_IN = os.environ.get("LOQA_PCM_STREAM_IN", "1") != "0"
# long-form audio: an utterance longer than 30 s is split into
# 30 s windows, encoded as extra encoder rows of the same batch (one
# cross-attention slot each) and decoded window after window, each window's
# decode prompted with the previous window's text (<|startofprev|>, at most
# PREV_TOKENS tokens, fed 4 per step like the SOT prompt); the texts are joined.
MAX_WINDOWS = int(os.environ.get("LOQA_STT_MAX_WINDOWS", "20"))
PREV_TOKENS = int(os.environ.get("LOQA_STT_PREV_TOKENS", "32"))
# admissions that may pass a waiting item that does not fit yet (FIFO otherwise)
HOL_BYPASS = int(os.environ.get("LOQA_STT_HOL_BYPASS", "16"))


def compression_ratio(text: str) -> float:
    """Whisper's repetition measure of a window's text: UTF-8 bytes over their
    zlib-compressed size (1.0 for empty text). A phrase repeated over and over
    compresses well: a ratio above ~2.4 marks a repetition loop."""
    b = text.encode("utf-8")
    return len(b) / len(zlib.compress(b)) if b else 1.0


def needs_fallback(text: str, mean_logprob: float | None, compression_ratio_threshold: float,
                   logprob_threshold: float) -> bool:
    """Whisper's ``decode_with_fallback`` test of one decoded window: too
    repetitive, or its mean token log-probability too low."""
    if compression_ratio(text) > compression_ratio_threshold:
        return True
    return mean_logprob is not None and mean_logprob < logprob_threshold


def check_temperatures(temperatures) -> tuple:
    """The fallback schedule as a tuple of floats: first entry 0, strictly
    increasing, all within [0, 1]."""
    try:
        t = tuple(float(x) for x in temperatures)
    except (TypeError, ValueError):
        raise ValueError(f"STT temperatures {temperatures!r}: a sequence of numbers") from None
    if not t or t[0] != 0.0 or any(not 0.0 <= x <= 1.0 for x in t) or \
            any(b <= a for a, b in zip(t, t[1:])):
        raise ValueError(f"STT temperatures {t}: strictly increasing from 0 within [0, 1]")
    return t


def n_windows(n_samples: int, cap: int = MAX_WINDOWS) -> int:
    """30 s windows of an utterance, at most ``cap`` (an engine passes
    min(MAX_WINDOWS, max_batch): every window holds a cross-attention slot, so
    a longer utterance is truncated like one past MAX_WINDOWS, not rejected)."""
    return max(1, min(cap, -(-n_samples // N_SAMPLES)))


@dataclass(eq=False)
class STTRequest:
    pcm: np.ndarray                   # int16 samples at ``sample_rate``
    transcript: str | None = None     # teacher-forcing target (synthetic mode)
    max_new_tokens: int = 96          # per 30 s window
    staged: object = None             # pinned PCM slot (engine/pcm_staging.py) holding the samples
    n_samples: int = 0                # 16 kHz samples transcribed (<= MAX_WINDOWS x 30 s)
    # the rate ``pcm`` / ``staged`` were recorded at (ops.RESAMPLE_RATES); other
    # than 16 kHz: resampled on the device by the upload's convert launch
    sample_rate: int = 16000
    # teacher-forcing targets per 30 s window of a long-form utterance (else
    # ``transcript`` is split over the windows by words)
    transcript_windows: list | None = None
    # outputs
    text: str = ""
    sumsq: float = 0.0
    rms: float = 0.0
    tokens: list[int] = field(default_factory=list)
    # STTEngine(token_logprobs=True), free decoding: the log-probability of each
    # entry of ``tokens`` (the window being decoded; a sampled EOT included) and
    # the mean over every sampled token of every window (Whisper's avg_logprob).
    # Teacher-forced requests emit their target, not the sample: empty / None.
    logprobs: list[float] = field(default_factory=list)
    avg_logprob: float | None = None
    # STTEngine(sot_probe=True): the language read from the start-of-transcript
    # logits (code; with a fixed language that one) and its probability among
    # the candidate languages, Whisper's no_speech_prob of every 30 s window and
    # their minimum (the utterance is silent only if every window is)
    language: str | None = None
    language_prob: float | None = None
    no_speech_probs: list[float] = field(default_factory=list)
    no_speech_prob: float | None = None
    # STTEngine(timestamps=True), free decoding (None with the feature off):
    # ``segments`` = (start_s, end_s, text) in utterance time (window w adds
    # 30 w s; ends clamped to the utterance's duration), the first segment's
    # start and the last one's end, and the windows whose last segment never got
    # its closing timestamp (cut by the window edge, EOT or the token limit)
    segments: list | None = None
    speech_start_s: float | None = None
    speech_end_s: float | None = None
    open_segments: list | None = None
    # STTEngine(temperatures=(0, ...)): the key of every random draw of this
    # request is (sample_seed, window, attempt, token index); None: the engine
    # assigns one. Per window, the temperature of the attempt that was kept and
    # its text's compression ratio; the attempts that were discarded in all.
    sample_seed: int | None = None
    temperatures: list = field(default_factory=list)
    compression_ratios: list = field(default_factory=list)
    fallback_attempts: int = 0
    # STTEngine(word_timestamps=True) (None with the feature off): ``words`` =
    # (start_s, end_s, word, probability) in utterance time (window w adds 30 w s,
    # clamped to the utterance's duration; probability None when teacher-forced),
    # ``word_segments`` the index of each word's segment (with timestamps off: its
    # window), ``token_frames`` per kept window the raw ``tok_frame`` of its text
    # tokens (and of a sampled EOT), 20 ms frames from the window's start
    words: list | None = None
    word_segments: list | None = None
    token_frames: list = field(default_factory=list)
    # STTEngine(beam_size=B > 1), free decoding: the beam width the request was
    # decoded with (1: greedy, and every teacher-forced request), the last
    # window's hypotheses as (tokens, sum_logprob), the winner (the highest
    # sum_logprob / text tokens; it is ``tokens`` / ``logprobs``) first, and
    # the same list for every window. A hypothesis that ended in EOT includes it.
    beam_size: int = 1
    hypotheses: list = field(default_factory=list)
    window_hypotheses: list = field(default_factory=list)
    seq_id: int = -1
    t_done: float = 0.0
    t_enc0: float = 0.0               # encoder start / end, decoder start (perf_counter)
    t_enc1: float = 0.0
    t_dec0: float = 0.0
    # decoder state (engine-owned)
    slot: int = -1                    # cross-attention K|V slot (encoder rows)
    target: list[int] | None = None
    feed: list[int] = field(default_factory=list)
    step: int = 0
    on_done: object = None
    # long-form state (engine-owned): windows, the one being decoded, their
    # cross-attention slots, finished windows' texts / tokens, prompt steps
    windows: int = 1
    win: int = 0
    slots: list = field(default_factory=list)
    win_texts: list = field(default_factory=list)
    prev_tokens: list = field(default_factory=list)
    prompt_steps: int = 1
    # the window's prompt as the feeds of its first ``prompt_steps`` steps (a
    # probing engine appends the last one when the SOT step has retired)
    chunks: list = field(default_factory=list)
    sot_step: int = -1                # probing engine: the step whose feed ends in SOT
    sot_pending: bool = False         # ... and its result has not been read yet
    lang_id: int = -1                 # the language token fed after SOT
    gated_windows: int = 0            # windows dropped by the no-speech rule
    lp_sum: float = 0.0               # finished windows' log-probability sum / count
    lp_n: int = 0
    attempt: int = 0                  # index into the engine's temperatures (this window)
    prompt_len: int = 0               # tokens fed before the window's first sampled token
    beam: object = None               # the window's BeamGroup while it is searched (stt_beam.py)
    # debug: per beam the tokens its row is made to follow (parents forced to
    # the identity), and per hypothesis the source row of each of its tokens
    beam_force: list | None = None
    # STTEngine(hotwords=[...]) (None with the feature off): the phrases whose
    # token sequence occurs in the kept windows' text tokens, in order of first
    # occurrence
    hotwords: list | None = None
    hypothesis_traces: list = field(default_factory=list)
    # where each window starts in the utterance, seconds: 30 w for the fixed
    # 30 s windows, the plan's ``a * 0.02`` with VAD (set by ``upload``)
    win_starts: list = field(default_factory=list)
    # STTEngine(vad=VadConfig(...)), free decoding (None / False with the
    # feature off and for teacher-forced requests): the detector's speech spans
    # as (start_s, end_s) in utterance time, clamped to the duration; the speech
    # they hold in seconds; ``vad_silent``: no span at all - the utterance took
    # no encoder row and no decoder step, its text is empty and ``windows`` is 0
    vad_spans: list | None = None
    vad_speech_s: float | None = None
    vad_silent: bool = False
    # engine-owned: the window plan, (a, b) in 20 ms frames per window (None:
    # fixed 30 s windows)
    win_frames: list | None = None


class STTEngine:
    SEQ_BUCKETS = [1, 2, 4, 8, 16, 32, 64, 128]
    SPLIT_KEYS = 128
    # int32 metadata of a captured decoder step, in staging order (engine/step_io.py)
    STEP_FIELDS = ("tokens", "positions", "slots", "cu_q", "ctx_lens", "block_tables",
                   "enc_starts", "enc_lens", "src", "row_slot")

    @classmethod
    def step_layout(cls, B_pad: int, T_pad: int, max_blocks: int) -> StepLayout:
        return StepLayout(step_shapes(cls.STEP_FIELDS, B_pad, T_pad, max_blocks),
                          max(16, ops.mpad_for(B_pad)))

    def __init__(self, cfg: WhisperConfig, device, *, seed: int = 0, max_batch: int = 64,
                 block_size: int = 16, use_graphs: bool = True, fast_decode: bool = True,
                 fused: bool = True, weights: WhisperWeights | None = None,
                 contended_tuning: bool = False, tokenizer=None, language: str = "en",
                 token_logprobs: bool = False, sot_probe: bool = False,
                 languages: list[str] | None = None, no_speech: bool = False,
                 no_speech_threshold: float = 0.6, logprob_threshold: float = -1.0,
                 timestamps: bool = False, max_initial_timestamp: float = 1.0,
                 temperatures=(0.0,), compression_ratio_threshold: float = 2.4,
                 word_timestamps: bool = False, alignment_heads=None, beam_size: int = 1,
                 hotwords=None, hotword_boost: float = 2.0, vad=None):
        self.cfg = cfg
        # voice activity detection (engine/stt_vad.py): ``upload`` runs ops.vad
        # over the PCM of the freely decoded utterances once it is on the device,
        # reads the speech spans back and builds the encoder rows from a window
        # plan that starts and ends at speech and cuts at pauses; an utterance
        # without speech takes no encoder row. None: off - no field, no buffer,
        # no launch and no host read beyond the plain engine's.
        from .stt_vad import VadConfig
        if vad is not None and not isinstance(vad, VadConfig):
            raise ValueError(f"STT vad: a VadConfig or None, not {type(vad).__name__}")
        self.vad = vad
        self.vad_params = vad.params if vad is not None else None
        self._vad_host = None           # pinned read-back buffer, grown on demand
        # cross-attention slots a VAD plan did not need, handed back by the
        # encoder thread and reclaimed by the scheduler
        self._spare_slots: collections.deque = collections.deque()
        # hotword biasing (engine/hotwords.py): every decoder step ends, before
        # the sampler, with ops.hotword_step, which advances the sequence's node
        # of the phrase automaton by the token it sampled last (``hw_state`` and
        # ``last_tok``, per cross-attention slot on the device) and adds
        # ``hotword_boost`` to the logit of every token the node expects. What
        # the sampler reports (log-probabilities, the no-speech and fallback
        # tests on them) is computed from the biased logits. None / empty: off,
        # and fields, launches and results are the plain engine's.
        from .hotwords import check_boost, normalize_phrases
        hotwords = normalize_phrases(hotwords)
        self.hotwords_on = bool(hotwords)
        self.hotword_boost = check_boost(hotword_boost)
        if self.hotwords_on and int(beam_size) > 1:
            raise ValueError("STT beam_size > 1 does not combine with hotwords (hypotheses "
                             "change rows; their hotword state does not follow them)")
        # beam search (engine/stt_beam.py): Whisper's BeamSearchDecoder with
        # patience 1 over ``beam_size`` hypotheses per freely decoded window,
        # selected on the device (ops.beam_topk / beam_merge), the KV moved
        # between hypotheses by ops.kv_copy_blocks. 1: off, the greedy engine.
        self.beam_size = int(beam_size)
        if not 1 <= self.beam_size <= ops.BEAM_MAX:
            raise ValueError(f"STT beam_size {beam_size} is outside 1..{ops.BEAM_MAX}")
        if self.beam_size > 1 and (timestamps or word_timestamps or
                                   len(check_temperatures(temperatures)) > 1):
            raise ValueError("STT beam_size > 1 does not combine with timestamps, word "
                             "timestamps or a temperature fallback schedule")
        if self.beam_size > max_batch:
            raise ValueError(f"STT beam_size {beam_size} exceeds max_batch {max_batch} (rows)")
        # temperature fallback (Whisper's decode_with_fallback): a freely decoded
        # window whose text is too repetitive (compression_ratio_threshold) or too
        # improbable (logprob_threshold) is decoded again at the next temperature,
        # its tokens drawn on the device (ops.masked_argmax_sample). (0.0,): off,
        # the greedy engine as it was.
        self.temperatures = check_temperatures(temperatures)
        self.compression_ratio_threshold = float(compression_ratio_threshold)
        if not self.compression_ratio_threshold >= 0.0:
            raise ValueError("compression_ratio_threshold must be >= 0")
        self.fallback = len(self.temperatures) > 1
        self.seed = int(seed)
        self._seed_ctr = 0
        # language "auto" (or empty, as the reference passes an empty
        # STT_LANGUAGE through): the language is the argmax over the candidate
        # language tokens at the start-of-transcript position
        language = (language or "auto").strip().lower() or "auto"
        self.auto_language = language == "auto"
        self.language = None if self.auto_language else language
        # no_speech: Whisper's rule drops a freely decoded window whose
        # no_speech_prob > no_speech_threshold and whose mean token
        # log-probability < logprob_threshold
        self.no_speech = bool(no_speech)
        self.no_speech_threshold = float(no_speech_threshold)
        self.logprob_threshold = float(logprob_threshold)
        # the decoder reads the start-of-transcript logits (language and
        # no_speech_prob): SOT ends a step of its own, every step samples through
        # ops.masked_argmax_logprob_probe
        self.sot_probe = bool(sot_probe) or self.auto_language or self.no_speech
        # every step also returns the log-softmax (after the suppress mask) of
        # the token it samples (ops.masked_argmax_logprob); off: ops.masked_argmax
        # timestamps: the prompt drops <|notimestamps|> and every step samples
        # under Whisper's timestamp rules (ops.masked_argmax_timestamps), their
        # state per cross-attention slot in ``ts_state`` on the device
        self.timestamps = bool(timestamps)
        # the engine stages per-sequence sampling fields (mask_row, probe, with
        # timestamps ts_ctl) and a step returns three results
        self.row_fields = self.sot_probe or self.timestamps or self.fallback
        # (word timestamps report a probability per word: they record them too)
        token_logprobs = bool(token_logprobs) or self.row_fields or bool(word_timestamps) or \
            self.beam_size > 1
        self.token_logprobs = token_logprobs
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        from ..utils.streams import decode_cap, init_pools
        init_pools(self.device)       # fixed stream -> hardware-queue placement
        self.max_wgs = decode_cap("LOQA_STT_MAX_WGS")
        # optional: tune the decode GEMMs under a background weight stream
        # (ops.contended_tuning; measured noisier and 5 % slower end to end)
        with ops.decode_cap(self.max_wgs), ops.contended_tuning(self.device, contended_tuning):
            self.weights = weights or WhisperWeights(cfg, self.device, seed=seed)
        self.weights.max_wgs = self.max_wgs or ops.MAX_DECODE_WGS
        self.model = WhisperModel(self.weights)
        self.tok = tokenizer or get_tokenizer(cfg.vocab_size)
        if self.sot_probe and isinstance(self.tok, SyntheticTokenizer):
            self.tok = SyntheticWhisperTokenizer(self.tok)
        if self.timestamps:
            if isinstance(self.tok, (SyntheticTokenizer, SyntheticWhisperTokenizer)):
                self.tok = SyntheticTimestampTokenizer(self.tok)
            if not hasattr(self.tok, "timestamp_tokens"):
                raise ValueError("STT timestamps: the tokenizer has no timestamp tokens")
            self.ts_begin, self.ts_count = self.tok.timestamp_tokens()
            mit = float(max_initial_timestamp)
            if not 0.0 <= mit <= 30.0:
                raise ValueError(f"max_initial_timestamp {mit} s is outside [0, 30]")
            self.max_initial = min(self.ts_count - 1, int(round(mit / 0.02)))
        self.step_fields = self.STEP_FIELDS
        if self.sot_probe:
            self._init_probe(language, languages)
            language = self.lang_codes[0]      # placeholder in ``sot``: fed per request
        extra = ()
        if self.row_fields:
            extra = ("mask_row", "probe") + (("ts_ctl",) if self.timestamps else ()) + \
                (("temp", "rng") if self.fallback else ())
        if self.hotwords_on:
            extra += ("hw_ctl",)
        if extra:
            i = self.STEP_FIELDS.index("src")
            self.step_fields = self.STEP_FIELDS[:i] + extra + self.STEP_FIELDS[i:]
        # start-of-transcript prompt; the language token follows STT_LANGUAGE
        # (the reference passes it to its STT service)
        try:
            lang = self.tok.token_id(f"<|{language}|>")
        except KeyError:
            raise ValueError(f"STT language {language!r}: no <|{language}|> token in the "
                             "tokenizer (a multilingual Whisper tokenizer.json has one)") from None
        self.sot = [self.tok.token_id("<|startoftranscript|>"), lang,
                    self.tok.token_id("<|transcribe|>"), self.tok.token_id("<|notimestamps|>")]
        if self.timestamps:
            self.sot.pop()      # Whisper's default mode: timestamps on
        self.eot = self.tok.token_id("<|endoftext|>")
        if self.timestamps and not self.eot < self.ts_begin:
            raise ValueError("STT timestamps: <|endoftext|> must lie below the timestamp tokens")
        self.n_prompt_tokens_per_step = len(self.sot)
        try:
            self.sop = self.tok.token_id("<|startofprev|>")
        except KeyError:
            self.sop = None     # no previous-text prompt for long-form windows
        # a checkpoint's tokenizer: greedy decoding never emits its special /
        # timestamp tokens or the generation config's suppress_tokens (as the
        # reference's STT service decodes); one packed mask row for every
        # sequence. The synthetic tokenizer of the random-init weights: none.
        self._sup = self._sup_rows = None
        if self.row_fields:
            # a table of two rows, picked per sequence by the step's ``mask_row``
            # field: 0 = the suppress mask (all ones for the synthetic tokenizer),
            # 1 = the candidate language tokens (the SOT step; a timestamps
            # engine that does not probe has row 0 alone)
            from ..ops.reference import pack_mask
            row0 = self.tok.sampling_mask(keep=(self.eot,)) if hasattr(self.tok, "sampling_mask") \
                else torch.ones(cfg.vocab_size, dtype=torch.bool)
            rows = [row0]
            if self.sot_probe:
                row1 = torch.zeros(cfg.vocab_size, dtype=torch.bool)
                row1[self.lang_ids] = True
                rows.append(row1)
            self._sup = pack_mask(torch.stack(rows)).to(self.device)
        elif hasattr(self.tok, "sampling_mask"):
            from ..ops.reference import pack_mask
            self._sup = pack_mask(self.tok.sampling_mask(keep=(self.eot,))[None]).to(self.device)
            self._sup_rows = torch.zeros(max(256, 2 * max_batch), dtype=torch.int32,
                                         device=self.device)
        self.block_size = block_size
        self.max_blocks = (cfg.n_text_ctx + block_size - 1) // block_size
        self.kv = PagedKVCache(cfg.dec_layers, cfg.n_heads, cfg.head_dim,
                               max_batch * self.max_blocks + 8, block_size, self.device)
        self.is_gpu = self.device.type == "cuda"
        self.ws = ops.AttnWorkspace(self.device, max_batch * 8, cfg.n_heads, cfg.head_dim,
                                    max((cfg.n_audio_ctx + 255) // 256, (cfg.n_text_ctx + 255) // 256)
                                    ) if self.is_gpu else None
        self._next = 1
        self.stats = {"utterances": 0, "decode_steps": 0, "host_pre_s": 0.0, "gpu_wait_s": 0.0,
                      "encode_s": 0.0}
        if token_logprobs:
            self.stats.update(logprob_tokens=0, logprob_sum=0.0)
        if self.sot_probe:
            self.stats.update(no_speech_windows=0, no_speech_utterances=0, languages={})
        if self.timestamps:
            self.stats.update(timestamp_segments=0, open_segments=0)
        if self.fallback:
            self.stats.update(fallback_windows=0, fallback_attempts=0)
        if self.beam_size > 1:
            self.stats.update(beam_windows=0, beam_kv_copies=0)
        if self.vad is not None:
            self.stats.update(vad_utterances=0, vad_silent_utterances=0, vad_plan_fallbacks=0,
                              vad_windows_saved=0)
        self.hw_table = self.hw_auto = None
        self._live_reqs = None
        if self.hotwords_on:
            # the automaton node of every cross-attention slot (+ a trash slot,
            # the last), beside ``last_tok``, which a hotword engine always keeps
            self.stats.update(hotword_windows=0, hotword_matches=0)
            # the requests being decoded (set_hotwords waits for none); weak, so
            # a request its caller abandons does not count for ever
            self._live_reqs = weakref.WeakSet()
            self.hw_state = torch.zeros(max_batch + 1, dtype=torch.int32, device=self.device)
            self.last_tok = torch.zeros(max_batch + 1, dtype=torch.int32, device=self.device)
            self.hw_table = ops.HotwordTable(self.device)
            self.set_hotwords(hotwords)
        if self.timestamps:
            # the rule state of every cross-attention slot (+ a trash slot, the
            # last, for padding rows), beside ``last_tok``
            self.ts_state = torch.zeros(max_batch + 1, dtype=torch.int32, device=self.device)
        # word timestamps (Whisper's find_alignment without a second decoder
        # pass): every decoder step ends with ops.align_record, which keeps the
        # alignment heads' cross-attention queries per (slot, position); a kept
        # window is aligned in _finish (ops.align_scores / align_cost / dtw).
        # Record and alignment run on this engine's one stream.
        self.align = None
        if word_timestamps:
            if isinstance(alignment_heads, (list, tuple)):
                alignment_heads = ",".join(f"{int(l)}:{int(h)}" for l, h in alignment_heads)
            heads = ops.ref.alignment_heads(cfg.dec_layers, cfg.n_heads, alignment_heads,
                                            getattr(self.tok, "generation_config", None))
            self.align = ops.AlignStore(cfg, heads, max_batch + 1, self.device)
            self.stats.update(aligned_windows=0, aligned_words=0)
        self.max_batch = max_batch
        self.fast_decode = fast_decode
        # fused-epilogue decoder GEMMs (8 launches per layer) for Mpad <= 64
        self.fused = fused and fast_decode
        self.scratch = ops.FusedScratch(self.device) if self.fused else None
        self.use_graphs = use_graphs and self.is_gpu and fast_decode
        self.self_splits = (cfg.n_text_ctx + self.SPLIT_KEYS - 1) // self.SPLIT_KEYS
        # cross-attention keys per split (the workspace holds n_audio_ctx / 128 splits)
        self.cross_split_keys = max(self.SPLIT_KEYS,
                                    int(os.environ.get("LOQA_XATTN_SPLIT_KEYS", "256")) // 32 * 32)
        if fast_decode and self.is_gpu:
            self.ws = ops.AttnWorkspace(self.device, 128, cfg.n_heads, cfg.head_dim,
                                        max(self.self_splits, (cfg.n_audio_ctx + self.SPLIT_KEYS - 1)
                                            // self.SPLIT_KEYS))
        # cross-attention K|V of every decoder layer for up to max_batch
        # utterances, written in place each batch (graph-captured steps read it)
        # (with the layer-concatenated weights: one [rows, L * 2d] buffer whose
        # column blocks are the layers' K|V, written by one tiled GEMM per batch)
        self.xkv_all = None
        if getattr(self.weights, "xkv_all", None) is not None:
            self.xkv_all = torch.empty(max_batch * cfg.n_audio_ctx, cfg.dec_layers * 2 * cfg.d_model,
                                       dtype=torch.bfloat16, device=self.device)
            d2 = 2 * cfg.d_model
            self.xkv = [self.xkv_all[:, i * d2:(i + 1) * d2] for i in range(cfg.dec_layers)]
        else:
            self.xkv = [torch.empty(max_batch * cfg.n_audio_ctx, 2 * cfg.d_model, dtype=torch.bfloat16,
                                    device=self.device) for _ in range(cfg.dec_layers)]
        self._graphs: dict[tuple[int, int], dict] = {}
        self._graphs_frozen = False     # see LLMEngine: no capture while serving
        self._enc_graphs: dict = {}
        self._enc_graph_pool = None
        # token budget of one decoder step (each new sequence feeds the 4-token
        # SOT prompt; 17+ simultaneous arrivals would exceed ops.MPADS rows)
        self.step_tokens = max(len(self.sot), min(int(os.environ.get("LOQA_STT_STEP_TOKENS", "64")),
                                                  ops.MPADS[-2]))
        self._rr = 0
        if self.use_graphs:
            # step I/O without copy-engine operations between step graphs, as the
            # LLM engine (engine/step_io.py): its staging rows hold the largest
            # bucket; the last token of every cross-attention slot (+ a trash
            # slot) feeds the device-fed greedy steps, and with ``token_logprobs``
            # the tokens' log-probabilities are published beside them
            b_max = next((b for b in self.SEQ_BUCKETS if b >= max_batch), self.SEQ_BUCKETS[-1])
            if not self.hotwords_on:
                self.last_tok = torch.zeros(max_batch + 1, dtype=torch.int32, device=self.device)
            self.io = StepIO(self.device, self._layout(b_max, ops.MPADS[-1]), self.last_tok,
                             logprobs=2 if self.row_fields else token_logprobs)
        # two decoder steps in flight (the host prepares step j+1 while step j
        # runs); LOQA_STT_PIPELINE=0: one synchronous step at a time
        self.pipelined = self.use_graphs and os.environ.get("LOQA_STT_PIPELINE", "1") != "0"
        # the beam engine: one synchronous eager-launch step at a time; a list
        # in ``beam_debug`` collects every search step's beam_topk outputs
        self._beam = None
        self.beam_debug = None
        if self.beam_size > 1:
            from .stt_beam import BeamDecoder
            self.pipelined = False
            self.step_tokens = max(self.step_tokens, self.beam_size)
            self._beam = BeamDecoder(self)

    def _init_probe(self, language: str, languages: list[str] | None) -> None:
        """Tokens of the start-of-transcript probe: ``nospeech`` and the
        candidate languages (``lang_codes`` / ``lang_ids``, in token order; a
        fixed language: that one alone)."""
        tok = self.tok
        self.nospeech = None
        for name in ("<|nospeech|>", "<|nocaptions|>"):
            try:
                self.nospeech = tok.token_id(name)
                break
            except KeyError:
                pass
        if self.nospeech is None:
            raise ValueError("STT start-of-transcript probe: the tokenizer has neither "
                             "<|nospeech|> nor <|nocaptions|>")
        known = tok.language_tokens() if hasattr(tok, "language_tokens") else {}
        want = [language] if not self.auto_language else \
            [str(c).strip().lower() for c in languages] if languages else list(known)
        if not want:
            raise ValueError("STT language detection: the tokenizer has no language tokens")
        for c in want:
            if c not in known:
                raise ValueError(f"STT language {c!r}: no <|{c}|> token in the tokenizer "
                                 "(a multilingual Whisper tokenizer.json has one)")
        pairs = sorted({(known[c], c) for c in want})
        self.lang_ids = [i for i, _ in pairs]
        self.lang_codes = [c for _, c in pairs]
        self._lang_code = dict(pairs)

    def _layout(self, B_pad: int, T_pad: int) -> StepLayout:
        """``step_layout`` of this engine (a probing one stages two more
        per-sequence fields, ``mask_row`` and ``probe``; a timestamps one those
        and ``ts_ctl``; a temperature-fallback one ``temp`` and ``rng`` too; a
        hotword one ``hw_ctl``)."""
        if self.step_fields is self.STEP_FIELDS:
            return self.step_layout(B_pad, T_pad, self.max_blocks)
        return StepLayout(step_shapes(self.step_fields, B_pad, T_pad, self.max_blocks),
                          max(16, ops.mpad_for(B_pad)))

    # ------------------------------------------------------------ front end
    def upload(self, reqs: list[STTRequest], device_pcm: torch.Tensor | None = None
               ) -> tuple[torch.Tensor, torch.Tensor]:
        """PCM16 of all utterances -> device -> fused convert + pad + sum of
        squares kernel -> [B, 480000] f32 (the 30 s window).

        GPU: every request's samples sit in a pinned stager slot (the relay's
        chunks were appended there as they arrived; numpy requests are staged
        here), each slot goes to HBM with one hipMemcpyAsync on the stager's
        H2D stream, and this (compute) stream waits on the copies' events.
        ``device_pcm`` (already on the GPU, e.g. scattered by the DP router
        over RCCL) holds the concatenated samples and skips the copies.

        A request recorded at another rate (``STTRequest.sample_rate``) is
        uploaded as it is and resampled to 16 kHz by the convert launch: when
        any request of the batch is not 16 kHz the launch is
        ``ops.pcm16_resample_padded`` (one for the whole batch, 16 kHz requests
        pass through), otherwise ``ops.pcm16_to_f32_padded`` as ever. Windows,
        ``n_samples`` and the dropped-sample count are in 16 kHz samples.

        An engine with ``vad``: the freely decoded requests of the batch go
        through ``ops.vad`` once the PCM is on the device, their spans are read
        back once and their rows follow the window plan (``_vad_plan``): window
        ``(a, b)`` is the 16 kHz samples [320 a, min(320 b, n)) of the
        utterance, a silent utterance has no row. Such a batch is converted by
        ``ops.pcm16_resample_padded`` whatever its rates; a batch without a VAD
        request launches what the plain engine launches. The returned sums of
        squares (and ``STTRequest.sumsq`` / ``rms`` made of them) are those of
        the rows actually written: with VAD, of the planned windows only."""
        lens = []
        for r in reqs:
            n = self._n_out(r)          # everything below counts 16 kHz samples
            w = n_windows(n, self.max_windows)
            if n > w * N_SAMPLES:
                self.stats["long_form_dropped_samples"] = \
                    self.stats.get("long_form_dropped_samples", 0) + n - w * N_SAMPLES
                log.error("utterance of %.1f s exceeds %d windows (LOQA_STT_MAX_WINDOWS, "
                          "max_batch): the last %.1f s are not transcribed", n / 16000,
                          self.max_windows, (n - w * N_SAMPLES) / 16000)
            lens.append(min(n, w * N_SAMPLES))
            r.windows = w
            r.win_starts = [30.0 * i for i in range(w)]
            r.win_frames, r.vad_spans, r.vad_speech_s, r.vad_silent = None, None, None, False
        for r, n in zip(reqs, lens):
            r.n_samples = n
        rates = [r.sample_rate or 16000 for r in reqs]
        resampled = any(sr != 16000 for sr in rates)
        assert not (resampled and device_pcm is not None), "device_pcm is 16 kHz"
        out_lens = lens
        if resampled:
            # source samples uploaded per request: its own for 16 kHz, else what
            # the kept outputs' filter taps reach (all of them unless truncated)
            lens = [n if sr == 16000 else min(self._n_samples(r), self._src_reach(n, sr))
                    for r, n, sr in zip(reqs, out_lens, rates)]
        offs = np.zeros(len(reqs) + 1, np.int64)
        offs[1:] = np.cumsum(lens)
        # one padded 30 s encoder row per window: a request's windows are
        # consecutive slices of its samples, so the rows' offsets are the
        # cumulative row lengths
        row_lens = [min(N_SAMPLES, n - w * N_SAMPLES) for r, n in zip(reqs, out_lens)
                    for w in range(r.windows)]
        row_offs = np.zeros(len(row_lens) + 1, np.int64)
        row_offs[1:] = np.cumsum(row_lens)
        if device_pcm is not None:
            pcm = device_pcm[: int(offs[-1])]
        elif self.is_gpu:
            pcm = torch.empty(max(1, int(offs[-1])), dtype=torch.int16, device=self.device)
            cur = torch.cuda.current_stream(self.device).cuda_stream
            stager = self._stager()
            for r, o, n in zip(reqs, offs[:-1], lens):
                slot = r.staged if r.staged is not None else (
                    stager.stage(r.pcm) if PCM_STAGER else None)
                if slot is None:        # every pinned slot busy: a one-off pinned copy
                    h = torch.from_numpy(np.ascontiguousarray(r.pcm[:n], np.int16)).pin_memory()
                    pcm[int(o):int(o) + n].copy_(h, non_blocking=True)
                    continue
                slot.upload(pcm.data_ptr() + int(o) * 2, n, cur)
                r.staged = None
        else:
            pcm = torch.from_numpy(np.concatenate(
                [np.asarray(self._host_samples(r)[:n], np.int16) for r, n in zip(reqs, lens)]
                or [np.zeros(0, np.int16)]))
            for r in reqs:
                if r.staged is not None:
                    r.staged.release()
                    r.staged = None
        if self.vad is not None and self._vad_plan(reqs, pcm, offs, lens, out_lens, rates):
            # rows from the window plans (teacher-forced requests: fixed windows)
            rows = []
            for r, o, n_src, n, sr in zip(reqs, offs[:-1], lens, out_lens, rates):
                wins = r.win_frames if r.win_frames is not None else \
                    [(w * 1500, (w + 1) * 1500) for w in range(r.windows)]
                rows += [(int(o), n_src, a * 320, min(b * 320, n) - a * 320, sr) for a, b in wins]
            return ops.pcm16_resample_padded(pcm, rows, N_SAMPLES)
        if resampled:
            # one launch for the whole batch: a row is a 30 s window of its
            # utterance's 16 kHz signal (16 kHz utterances pass through)
            rows = [(int(o), n_src, w * N_SAMPLES, min(N_SAMPLES, n - w * N_SAMPLES), sr)
                    for r, o, n_src, n, sr in zip(reqs, offs[:-1], lens, out_lens, rates)
                    for w in range(r.windows)]
            return ops.pcm16_resample_padded(pcm, rows, N_SAMPLES)
        off_t = torch.from_numpy(row_offs)
        if self.is_gpu:
            off_t = off_t.pin_memory().to(self.device, non_blocking=True)
        return ops.pcm16_to_f32_padded(pcm, off_t, N_SAMPLES, row_offs)

    @staticmethod
    def _n_samples(r: STTRequest) -> int:
        return len(r.staged) if r.staged is not None else len(r.pcm)

    @classmethod
    def _n_out(cls, r: STTRequest) -> int:
        """16 kHz samples of the request: ceil(n_src * 16000 / rate)."""
        n, sr = cls._n_samples(r), r.sample_rate or 16000
        return n if sr == 16000 else ops.ref.resample_len(n, ops.ref.check_rate(sr), 16000)

    @staticmethod
    def _src_reach(n_out: int, rate: int) -> int:
        """Source samples the first ``n_out`` 16 kHz outputs read."""
        _, L, M, T = ops.ref.resample_filter(rate, 16000)
        return 0 if n_out <= 0 else (n_out - 1) * M // L + (T - 1) // 2 + 1

    def _vad_plan(self, reqs: list[STTRequest], pcm: torch.Tensor, offs, lens, out_lens,
                  rates) -> bool:
        """``ops.vad`` over the freely decoded requests of an uploaded batch
        (request i is ``pcm[offs[i] : offs[i] + lens[i]]`` at ``rates[i]``, and
        ``out_lens[i]`` 16 kHz samples), one read-back of the spans through
        pinned memory, and each request's window plan: ``win_frames``,
        ``windows`` (0: silent), ``win_starts`` and the ``vad_*`` results.
        ``r.windows`` comes in as the slots admission reserved for it. False: the
        batch has no such request and nothing was launched."""
        from .stt_vad import FRAME_HZ, clip_spans, plan_windows_counted, spans_seconds
        idx = [i for i, r in enumerate(reqs)
               if r.transcript is None and r.transcript_windows is None]
        if not idx:
            return False
        descs, f0 = [], 0
        for i in idx:
            descs.append((int(offs[i]), int(lens[i]), int(rates[i]), f0))
            f0 += ops.ref.vad_frames(lens[i], rates[i])
        U = len(idx)
        cap = max(ops.ref.vad_frames(d[1], d[2]) for d in descs) // 2 + 1
        # spans, n_spans and speech_frames in one buffer: one copy reads them all
        n_sp = U * cap * 2
        buf = torch.empty(n_sp + 2 * U, dtype=torch.int32, device=pcm.device)
        E = torch.zeros(max(f0, 1), dtype=torch.int32, device=pcm.device)
        ops.vad(pcm, descs, self.vad_params,
                out=(E, buf[:n_sp].view(U, cap, 2), buf[n_sp:n_sp + U], buf[n_sp + U:]))
        if self.is_gpu:
            if self._vad_host is None or self._vad_host.numel() < buf.numel():
                self._vad_host = torch.empty(max(4096, 2 * buf.numel()),
                                             dtype=torch.int32).pin_memory()
            host = self._vad_host[: buf.numel()]
            host.copy_(buf, non_blocking=True)
            torch.cuda.current_stream(self.device).synchronize()
            h = host.numpy()
        else:
            h = buf.numpy()
        spans = h[:n_sp].reshape(U, cap, 2)
        n_spans, speech = h[n_sp:n_sp + U], h[n_sp + U:]
        for u, i in enumerate(idx):
            r, n = reqs[i], out_lens[i]
            dur = n / 16000.0
            sp = clip_spans(spans[u, : int(n_spans[u])].tolist(), -(-n // 320))
            reserved = r.windows
            plan, fell_back = plan_windows_counted(sp, reserved)
            self.stats["vad_utterances"] += 1
            self.stats["vad_plan_fallbacks"] += fell_back
            self.stats["vad_windows_saved"] += reserved - len(plan)
            r.win_frames = plan
            r.windows = len(plan)
            r.win_starts = [a / FRAME_HZ for a, _ in plan]
            r.vad_spans = spans_seconds(sp, dur)
            r.vad_speech_s = min(int(speech[u]) / FRAME_HZ, dur)
            r.vad_silent = not plan
        return True

    @staticmethod
    def _host_samples(r: STTRequest) -> np.ndarray:
        return r.staged.numpy() if r.staged is not None else r.pcm

    def _stager(self):
        """The engine's pinned PCM stager (created on first use)."""
        if getattr(self, "stager", None) is None:
            from .pcm_staging import PcmStager
            h2d = None
            if PCM_STREAM_IN:
                from ..utils.streams import placed_stream
                h2d = placed_stream(self.device, "h2d")
            self.stager = PcmStager(2 * self.max_batch + 16, N_SAMPLES, h2d_stream=h2d)
        return self.stager

    def new_pcm_slot(self):
        """A pinned slot for one relay's incoming PCM (None: CPU engine or every
        slot busy - the caller then buffers on the host)."""
        if not self.is_gpu:
            return None
        return self._stager().acquire()

    # -------------------------------------------------------------- decode
    def cross_kv(self, enc: torch.Tensor, slots: list[int] | None = None) -> list[torch.Tensor]:
        """Cross-attention K|V of every decoder layer for the encoder rows of
        ``enc`` ([n * T_enc, d]), written to the requests' slots (default:
        slots 0..n-1, one GEMM per layer; contiguous slot runs share a GEMM)."""
        T = self.cfg.n_audio_ctx
        n = enc.shape[0] // T
        slots = list(range(n)) if slots is None else slots
        assert max(slots) < self.max_batch, "slot exceeds max_batch"
        runs, i = [], 0                     # (first request, first slot, length)
        while i < n:
            j = i
            while j + 1 < n and slots[j + 1] == slots[j] + 1:
                j += 1
            runs.append((i, slots[i], j - i + 1))
            i = j + 1
        if self.xkv_all is not None:
            w = self.weights
            for i0, s0, m in runs:
                ops.gemm_tile(enc[i0 * T:(i0 + m) * T], w.xkv_all, bias=w.xkv_all_b,
                              out=self.xkv_all[s0 * T:(s0 + m) * T], layout=7)
            return self.xkv
        for L, buf in zip(self.weights.dec, self.xkv):
            for i0, s0, m in runs:
                torch.addmm(L["xkv_b"], enc[i0 * T:(i0 + m) * T], L["xkv"].t(),
                            out=buf[s0 * T:(s0 + m) * T])
        return self.xkv

    def _host_meta(self, live: list[STTRequest], B_pad: int, T_pad: int,
                   out: dict | None = None, feeds: list | None = None,
                   sot: list | None = None, ts_ctl: list | None = None,
                   samp: list | None = None) -> tuple[int, dict]:
        """Host metadata of one step feeding ``feeds`` (default: every
        request's ``feed``); ``out`` = preallocated views (a staging row) to
        fill in place and return. ``sot`` (probing engine): the requests whose
        feed ends in SOT this step (default: ``sot_pending`` and the whole
        remaining prompt fed). ``ts_ctl`` (timestamps or hotword engine): the
        rows' rule control words, staged as ``ts_ctl`` and / or ``hw_ctl``
        (default: ``_ts_ctl`` of a step that feeds every request's whole
        remaining feed). ``samp`` (temperature fallback): the rows'
        (temperature, random key) (default: ``_samp`` of such a step)."""
        T_enc = self.cfg.n_audio_ctx
        if feeds is None:
            feeds = [r.feed for r in live]
        host = fill_meta(self.kv.pool, [r.seq_id for r in live], feeds, B_pad, T_pad,
                         self.max_blocks, max(16, ops.mpad_for(B_pad)), out, "STT KV cache")
        if out is None:
            host["enc_starts"] = np.zeros(B_pad, np.int32)
            host["enc_lens"] = np.zeros(B_pad, np.int32)
        n = len(live)
        enc_starts, enc_lens = host["enc_starts"], host["enc_lens"]
        enc_starts[:n] = [r.slot * T_enc for r in live]
        enc_starts[n:] = 0
        enc_lens[:n] = T_enc
        enc_lens[n:] = 0
        if self.row_fields:
            if sot is None:
                sot = [r.sot_pending and len(f) == len(r.feed) for r, f in zip(live, feeds)]
            if out is None:
                host["mask_row"] = np.zeros(B_pad, np.int32)
                host["probe"] = np.zeros(B_pad, np.int32)
            mask_row, probe = host["mask_row"], host["probe"]
            mask_row[:n] = [1 if x else 0 for x in sot]
            mask_row[n:] = 0
            probe[:n] = [self.nospeech if x else -1 for x in sot]
            probe[n:] = -1
        if (self.timestamps or self.hotwords_on) and ts_ctl is None:
            ts_ctl = [self._ts_ctl(r, len(f) < len(r.feed)) for r, f in zip(live, feeds)]
        if self.hotwords_on:
            # the hotword control word is the timestamp rules': both say where
            # in its window's free decoding the row's step is
            if out is None:
                host["hw_ctl"] = np.zeros(B_pad, np.int32)
                host["row_slot"] = np.full(B_pad, self.max_batch, np.int32)
                host["row_slot"][:n] = [r.slot for r in live]
            host["hw_ctl"][:n] = ts_ctl
            host["hw_ctl"][n:] = 0
        if self.timestamps:
            if out is None:
                # an eager step: the graphs' callers stage ``row_slot`` themselves
                host["ts_ctl"] = np.zeros(B_pad, np.int32)
                host["row_slot"] = np.full(B_pad, self.max_batch, np.int32)
                host["row_slot"][:n] = [r.slot for r in live]
            host["ts_ctl"][:n] = ts_ctl
            host["ts_ctl"][n:] = 0
        if self.align is not None and out is None:
            host["row_slot"] = np.full(B_pad, self.max_batch, np.int32)
            host["row_slot"][:n] = [r.slot for r in live]
        if self.fallback:
            if samp is None:
                samp = [self._samp(r, len(f) < len(r.feed)) for r, f in zip(live, feeds)]
            if out is None:
                host["temp"] = np.zeros(B_pad, np.int32)
                host["rng"] = np.zeros(B_pad, np.int32)
            # the temperature travels as its f32 bits in the int32 block
            host["temp"][:n] = np.asarray([t for t, _ in samp], np.float32).view(np.int32)
            host["temp"][n:] = 0
            host["rng"][:n] = [k for _, k in samp]
            host["rng"][n:] = 0
        return max([len(f) for f in feeds] + [1]), host

    def _ts_ctl(self, r: STTRequest, partial: bool = False) -> int:
        """The timestamp-rule control word of ``r``'s next step, from what the
        host knows without seeing tokens: 0 = rules off (a prompt chunk whose
        logits are discarded - ``partial``: more of the prompt follows -, the SOT
        probe step, every step of a teacher-forced window: its targets carry no
        timestamps and the sampled token is not the one fed), 1 = the step that
        feeds the window's last prompt token, 2 = every later step."""
        if partial or r.sot_pending or r.target is not None:
            return 0
        return 1 if not r.tokens else 2

    def _samp(self, r: STTRequest, partial: bool = False) -> tuple[float, int]:
        """(temperature, random key) of ``r``'s next step, known without tokens
        like ``_ts_ctl``: (0, 0) - the greedy row - for a prompt chunk, the SOT
        probe step and a teacher-forced window, else ``_samp_at`` of the token
        the step samples."""
        if partial or r.sot_pending or r.target is not None:
            return 0.0, 0
        return self._samp_at(r, len(r.tokens))

    def _samp_at(self, r: STTRequest, i: int) -> tuple[float, int]:
        """(temperature, int32 bits of the random key) of token ``i`` of ``r``'s
        window at its current attempt; an attempt at temperature 0 is greedy."""
        T = self.temperatures[r.attempt]
        if T == 0.0:
            return 0.0, 0
        return T, ops.ref.key_i32(ops.ref.sample_key(r.sample_seed, r.win, r.attempt, i))

    def _dev(self, host: dict, dst: dict | None = None) -> dict:
        return to_device(host, self.device, dst)

    def _self_splits(self, ctx: int | None) -> int:
        """Self-attention key splits for a context bound (graph bucket)."""
        if ctx is None:
            return self.self_splits
        return max(1, min(self.self_splits, (ctx + self.SPLIT_KEYS - 1) // self.SPLIT_KEYS))

    def _argmax(self, logits: torch.Tensor):
        """Sampled tokens; with ``token_logprobs`` (tokens, their log-probabilities)."""
        fn = ops.masked_argmax_logprob if self.token_logprobs else ops.masked_argmax
        if self._beam is not None:
            self._beam.logits = logits
        if self._sup is None:
            return fn(logits)
        return fn(logits, self._sup, self._sup_rows[: logits.shape[0]])

    def _sample(self, logits: torch.Tensor, dev: dict):
        """``_argmax``; a probing engine: (tokens, log-probabilities, probed
        log-probabilities) under each sequence's mask row, the probe read from
        the step's ``probe`` field."""
        B = logits.shape[0]
        if self.hotwords_on:
            # in place on the step's logits: everything below sees them biased
            ops.hotword_step(logits, logits.shape[1], dev["hw_ctl"][:B], dev["row_slot"][:B],
                             self.hw_state, self.last_tok, self.hw_table)
        if not self.row_fields:
            return self._argmax(logits)
        if self._beam is not None:
            self._beam.logits = logits
        if self.fallback:
            # the rules (when on) plus a per-row temperature and random key: a
            # row at temperature 0 is the greedy one, bit for bit
            ts = self.timestamps
            return ops.masked_argmax_sample(
                logits, self._sup, dev["mask_row"][:B], dev["probe"][:B],
                dev["ts_ctl"][:B] if ts else None, self.ts_state if ts else None,
                dev["row_slot"][:B] if ts else None, self.ts_begin if ts else 0,
                self.ts_count if ts else 0, self.eot if ts else 0, self.max_initial if ts else 0,
                dev["temp"][:B].view(torch.float32), dev["rng"][:B])
        if self.timestamps:
            # the same three results under Whisper's timestamp rules: the rows'
            # ``ts_ctl`` switches them on, their state is ``ts_state[row_slot]``
            return ops.masked_argmax_timestamps(
                logits, self._sup, dev["mask_row"][:B], dev["probe"][:B], dev["ts_ctl"][:B],
                self.ts_state, dev["row_slot"][:B], self.ts_begin, self.ts_count, self.eot,
                self.max_initial)
        return ops.masked_argmax_logprob_probe(logits, self._sup, dev["mask_row"][:B],
                                               dev["probe"][:B])

    def _host(self, res, B: int | None = None):
        """A step's device result (``_sample``) as numpy, cut to B rows."""
        if self.row_fields:
            return tuple(x[:B].cpu().numpy() for x in res)
        if self.token_logprobs:
            return res[0][:B].cpu().numpy(), res[1][:B].cpu().numpy()
        return res[:B].cpu().numpy()

    def _fast_forward(self, dev: dict, max_q: int, B_pad: int, ctx: int | None = None):
        ns = self._self_splits(ctx)
        al = (self.align, dev["row_slot"]) if self.align is not None else None
        if self.fused and dev["tokens"].numel() <= 64:
            logits = decode_step_fused(self.model, dev["tokens"], dev["positions"], dev["slots"],
                                       dev["cu_q"], dev["ctx_lens"], dev["block_tables"], max_q,
                                       self.kv.k, self.kv.v, self.xkv, dev["enc_starts"],
                                       dev["enc_lens"], dev["logit_idx"], self.ws, self.scratch,
                                       ns, self.SPLIT_KEYS, self.cross_split_keys, align=al)
            return self._sample(logits[:B_pad, : self.cfg.vocab_size], dev)
        logits = decode_step_fast(self.model, dev["tokens"], dev["positions"], dev["slots"],
                                  dev["cu_q"], dev["ctx_lens"], dev["block_tables"], max_q,
                                  self.kv.k, self.kv.v, self.xkv, dev["enc_starts"],
                                  dev["enc_lens"], dev["logit_idx"], self.ws, ns,
                                  self.SPLIT_KEYS, align=al)
        return self._sample(logits[:B_pad, : self.cfg.vocab_size], dev)

    def _graph(self, B_pad: int, T_pad: int, ctx: int) -> dict:
        """Captured decode step for (sequence bucket, token bucket, context
        bucket): the attention grid is sized for the bucket's context, so no
        workgroups are spent on splits past the longest sequence. The graph's
        first node fills the step metadata from the pinned staging ring (taking
        a greedy sequence's fed token from ``last_tok`` on the device), its last
        node publishes the sampled tokens to the pinned result ring."""
        key = (B_pad, T_pad, ctx)
        g = self._graphs.get(key)
        if g is None:
            max_q = max(1, min(len(self.sot), T_pad))
            g = self._graphs[key] = self.io.capture(
                self._layout(B_pad, T_pad), T_pad,
                lambda dev: self._fast_forward(dev, max_q, B_pad, ctx))
        return g

    # encoder graphs for batches of up to this many utterances (0: eager encoder)
    ENC_GRAPH_MAX = 4

    def _enc_graph(self, B: int) -> dict:
        """The Whisper encoder (log-mel -> conv stem -> all layers) for a batch
        of B padded 30-s windows as ONE graph replay: ~330 kernels per encode
        launched eagerly from the encoder worker thread leave host-launch gaps
        between them (and hold the GIL the decoder schedulers need). The graphs
        share one memory pool; replays run on the encoder's stream one after
        another, so their intermediates never overlap in time."""
        g = self._enc_graphs.get(B)
        if g is not None:
            return g
        if self._enc_graph_pool is None:
            self._enc_graph_pool = torch.cuda.graph_pool_handle()
        audio = torch.zeros(B, 480000, dtype=torch.float32, device=self.device)
        s = torch.cuda.Stream(self.device)
        s.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(s):
            self.model.encode(audio)
        torch.cuda.current_stream(self.device).wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, pool=self._enc_graph_pool, capture_error_mode="thread_local"):
            out = self.model.encode(audio)
        g = {"graph": graph, "audio": audio, "out": out}
        self._enc_graphs[B] = g
        return g

    def encode(self, audio: torch.Tensor) -> torch.Tensor:
        """Encoder states [B * 1500, d] of padded audio [B, 480000]: a graph
        replay for a captured batch size, else the eager encoder."""
        B = audio.shape[0]
        g = self._enc_graphs.get(B)
        if g is None:
            return self.model.encode(audio)
        g["audio"].copy_(audio)
        g["graph"].replay()
        return g["out"]

    def warmup_graphs(self) -> int:
        """Capture every decoder-step graph bucket up front (see
        ``LLMEngine.warmup_graphs``): sequence x token x context buckets; and
        the encoder for batches of 1 .. ``ENC_GRAPH_MAX`` utterances."""
        if not self.use_graphs:
            return 0
        n = 0
        if self.is_gpu:
            for b in range(1, min(self.ENC_GRAPH_MAX, self.max_batch) + 1):
                self._enc_graph(b)
                n += 1
        # a timestamps engine's prompt is one token shorter (a graph's max_q
        # follows it); its bucket set is that of the full prompt all the same
        if self._beam is not None:      # beam steps launch eagerly: the encoder graphs alone
            return n
        buckets = decode_buckets(self.SEQ_BUCKETS, self.max_batch, self.step_tokens,
                                 len(self.sot) + int(self.timestamps), self.SPLIT_KEYS,
                                 self.cfg.n_text_ctx)
        for b, t, c in buckets:
            self._graph(b, t, c)
        self._graphs_frozen = True
        return n + len(buckets)

    def _step(self, live: list[STTRequest], sot: list | None = None, ts_ctl: list | None = None,
              samp: list | None = None):
        """One decoder step for every live request (its ``feed`` tokens): the
        sampled tokens, with ``token_logprobs`` (tokens, log-probabilities), a
        probing or timestamps engine (tokens, log-probabilities, probed
        log-probabilities). ``sot``, ``ts_ctl``, ``samp``: see ``_host_meta``."""
        B = len(live)
        T = sum(len(r.feed) for r in live)
        if self.fast_decode:
            B_pad = next((b for b in self.SEQ_BUCKETS if b >= B), B)
            T_pad = ops.mpad_for(T)
            ctx = max(self.kv.pool.seq_len(r.seq_id) + len(r.feed) for r in live)
            C = min(self.cfg.n_text_ctx, -(-ctx // self.SPLIT_KEYS) * self.SPLIT_KEYS)
            if self.use_graphs and self._beam is None and \
                    ((B_pad, T_pad, C) in self._graphs or not self._graphs_frozen):
                t0 = time.perf_counter()
                g = self._graph(B_pad, T_pad, C)
                hb = self.io.stage(g)
                self._host_meta(live, B_pad, T_pad, out=hb, sot=sot, ts_ctl=ts_ctl, samp=samp)
                hb["src"].fill(-1)
                hb["row_slot"].fill(self.io.trash)
                if self.timestamps or self.align is not None or self.hotwords_on:
                    # the rows' rule state / query store (and last_tok) slots
                    hb["row_slot"][:B] = [r.slot for r in live]
                t1 = time.perf_counter()
                rslot = self.io.replay(g)
                torch.cuda.current_stream(self.device).synchronize()
                out = self.io.result(rslot, B)
                self.stats["host_pre_s"] += t1 - t0
                self.stats["gpu_wait_s"] += time.perf_counter() - t1
                return out
            max_q, host = self._host_meta(live, B_pad, T_pad, sot=sot, ts_ctl=ts_ctl, samp=samp)
            res = self._fast_forward(self._dev(host), max_q, B_pad)
            self._keep_last(live, res)
            return self._host(res, B)
        if self.fallback:
            return self._eager_step(live, sot, ts_ctl, samp)
        if self.timestamps or self.hotwords_on:
            return self._eager_step(live, sot, ts_ctl)
        return self._eager_step(live, sot) if self.sot_probe else self._eager_step(live)

    def _keep_last(self, live: list[STTRequest], res) -> None:
        """A step outside the captured graphs has no publish node: a hotword
        engine writes the sampled tokens to ``last_tok`` itself, where the next
        step's ``ops.hotword_step`` reads them."""
        if not self.hotwords_on:
            return
        tok = res[0] if isinstance(res, tuple) else res
        idx = torch.tensor([r.slot for r in live], dtype=torch.long, device=self.device)
        self.last_tok[idx] = tok[: len(live)].to(torch.int32)

    def _eager_step(self, live: list[STTRequest], sot: list | None = None,
                    ts_ctl: list | None = None, samp: list | None = None):
        """Reference decode path (hipBLASLt GEMMs, eager launches)."""
        T_enc = self.cfg.n_audio_ctx
        toks, pos, slots, cu, ctx, lidx = [], [], [], [0], [], []
        bt = np.zeros((len(live), self.max_blocks), np.int32)
        max_q, max_ctx = 1, 1
        for j, r in enumerate(live):
            f = r.feed
            start = self.kv.pool.seq_len(r.seq_id)
            sl = self.kv.pool.append(r.seq_id, len(f))
            toks += f
            pos += list(range(start, start + len(f)))
            slots += sl
            cu.append(cu[-1] + len(f))
            ctx.append(start + len(f))
            tab = self.kv.pool.block_table(r.seq_id)
            bt[j, :len(tab)] = tab
            lidx.append(cu[-1] - 1)
            max_q = max(max_q, len(f))
            max_ctx = max(max_ctx, start + len(f))
        dev = lambda a, dt: torch.tensor(a, dtype=dt).to(self.device, non_blocking=True)
        enc_starts = dev([r.slot * T_enc for r in live], torch.int32)
        enc_lens = dev([T_enc] * len(live), torch.int32)
        al = (self.align, dev([r.slot for r in live], torch.int32)) \
            if self.align is not None else None
        logits = self.model.decode_step(
            dev(toks, torch.int32), dev(pos, torch.int32), dev(slots, torch.int32),
            dev(cu, torch.int32), dev(ctx, torch.int32), dev(bt, torch.int32), max_q, max_ctx,
            self.kv.k, self.kv.v, self.xkv, enc_starts, enc_lens, dev(lidx, torch.int64), self.ws,
            align=al)
        if not self.row_fields and not self.hotwords_on:
            return self._host(self._argmax(logits))
        meta = {}
        if (self.timestamps or self.hotwords_on) and ts_ctl is None:
            ts_ctl = [self._ts_ctl(r) for r in live]
        if self.hotwords_on:
            meta["hw_ctl"] = dev(list(ts_ctl), torch.int32)
            meta["row_slot"] = dev([r.slot for r in live], torch.int32)
        if self.row_fields:
            if sot is None:
                sot = [r.sot_pending for r in live]
            meta["mask_row"] = dev([1 if x else 0 for x in sot], torch.int32)
            meta["probe"] = dev([self.nospeech if x else -1 for x in sot], torch.int32)
        if self.timestamps:
            meta["ts_ctl"] = dev(list(ts_ctl), torch.int32)
            meta["row_slot"] = dev([r.slot for r in live], torch.int32)
        if self.fallback:
            if samp is None:
                samp = [self._samp(r) for r in live]
            meta["temp"] = dev([t for t, _ in samp], torch.float32).view(torch.int32)
            meta["rng"] = dev([k for _, k in samp], torch.int32)
        res = self._sample(logits, meta)
        self._keep_last(live, res)
        return self._host(res)

    # ----------------------------------------------------------- admission
    def _admit(self, reqs: list[STTRequest], slots: list[int],
               device_pcm: torch.Tensor | None = None) -> None:
        """Front end + encoder for newly arrived requests, their cross-attention
        K|V into ``slots``, and their decoder sequences (fed the SOT prompt)."""
        self._encode(reqs, slots, device_pcm)
        self._start_decode(reqs)

    def rows_needed(self, reqs: list[STTRequest]) -> int:
        """Encoder rows / cross-attention slots of ``reqs`` (one per 30 s window)."""
        return sum(n_windows(self._n_out(r), self.max_windows) for r in reqs)

    @property
    def max_slots(self) -> int:
        """Cross-attention slots in use at once: ``max_batch`` counts decoder
        rows, and a searched window holds ``beam_size`` of them."""
        return max(1, self.max_batch // self.beam_size)

    @property
    def max_windows(self) -> int:
        return max(1, min(MAX_WINDOWS, self.max_slots))

    def _encode(self, reqs: list[STTRequest], slots: list[int],
                device_pcm: torch.Tensor | None = None) -> None:
        """GPU half of admission (any thread with its own stream): PCM upload,
        log-mel + encoder, cross-attention K|V into the requests' slots (one per
        30 s window, in order); returns once that work is complete (the RMS
        read-back synchronises)."""
        tr = tracer()
        dev = self.device if self.is_gpu else None
        t_enc0 = time.perf_counter()
        with tr.span("h2d", dev, batch=len(reqs)):
            audio, sumsq = self.upload(reqs, device_pcm)
        t0 = time.perf_counter()
        # a VAD plan may need fewer rows than the slots reserved for the batch
        # (none at all when every utterance is silent: no encoder pass)
        slots, spare = list(slots[: audio.shape[0]]), list(slots[audio.shape[0]:])
        with tr.span("encode", dev, batch=len(reqs)):
            if slots:
                enc = self.encode(audio)
                self.cross_kv(enc, slots)
        ss = sumsq.cpu().numpy()
        if self.is_gpu:
            torch.cuda.current_stream(self.device).synchronize()
        t1 = time.perf_counter()
        self.stats["encode_s"] += t1 - t0
        for r in reqs:
            r.t_enc0, r.t_enc1 = t_enc0, t1
        i = 0
        for r in reqs:
            w = r.windows
            n = max(1, r.n_samples)
            r.sumsq = float(ss[i:i + w].sum())
            r.rms = float(np.sqrt(r.sumsq / n))
            r.slots = list(slots[i:i + w])
            r.slot = r.slots[0] if w else -1
            i += w
        self._spare_slots.extend(spare)

    def _reclaim_spare(self) -> None:
        """Slots a VAD plan left unused go back to the scheduler's free list."""
        if self._spare_slots:
            while self._spare_slots:
                self._free_slots.append(self._spare_slots.popleft())
            self._free_slots.sort()

    def _start_decode(self, reqs: list[STTRequest]) -> None:
        """Decoder sequences for encoded requests (scheduler thread)."""
        now = time.perf_counter()
        for r in reqs:
            r.t_dec0 = now
            r.t_done = 0.0
            r.win_texts, r.prev_tokens = [], []
            r.lp_sum, r.lp_n, r.avg_logprob = 0.0, 0, None
            r.language = r.language_prob = r.no_speech_prob = None
            r.no_speech_probs, r.lang_id, r.gated_windows = [], -1, 0
            r.segments = r.open_segments = r.speech_start_s = r.speech_end_s = None
            r.attempt, r.fallback_attempts = 0, 0
            r.temperatures, r.compression_ratios = [], []
            r.token_frames = []
            r.hypotheses, r.window_hypotheses, r.hypothesis_traces = [], [], []
            r.beam_size = self.beam_size if self._window_text(r, 0) is None else 1
            r.words, r.word_segments = ([], []) if self.align is not None else (None, None)
            if self.fallback and r.sample_seed is None:
                # a per-engine counter mixed with the engine seed
                self._seed_ctr += 1
                r.sample_seed = ops.ref.sample_key(self.seed, self._seed_ctr, 0, 0)
            if self.timestamps:
                r.segments, r.open_segments = [], []
            r.hotwords = [] if self.hotwords_on else None
            if r.vad_silent:
                # no span: no encoder row, no decoder sequence - done here
                r.text, r.tokens, r.logprobs = "", [], []
                r.t_done = time.perf_counter()
                self.stats["vad_silent_utterances"] += 1
                self.stats["utterances"] += 1
                continue
            if self._live_reqs is not None:
                self._live_reqs.add(r)
            if not r.slots:
                r.slots = [r.slot]
            self._begin_window(r, 0)

    def _window_text(self, r: STTRequest, w: int) -> str | None:
        """Teacher-forcing text of window ``w`` (None: free decoding)."""
        if r.transcript_windows is not None:
            return r.transcript_windows[w] if w < len(r.transcript_windows) else ""
        if r.transcript is None:
            return None
        if r.windows == 1:
            return r.transcript
        words = r.transcript.split()
        per = -(-len(words) // r.windows)
        return " ".join(words[w * per:(w + 1) * per])

    def _begin_window(self, r: STTRequest, w: int) -> None:
        """A fresh decoder sequence for window ``w`` of ``r`` over its encoder
        rows; later windows are prompted with the previous windows' text."""
        r.win = w
        r.slot = r.slots[w]
        r.beam = None
        r.seq_id = self._next
        self._next += 1
        self.kv.pool.add_seq(r.seq_id, [])
        prompt = []
        if w > 0 and self.sop is not None and r.prev_tokens and PREV_TOKENS > 0:
            prompt = [self.sop] + r.prev_tokens[-PREV_TOKENS:]
        r.tokens, r.step, r.feed = [], 0, prompt + list(self.sot)
        r.prompt_len = len(r.feed)
        r.logprobs = []
        c = len(self.sot)
        r.sot_step, r.sot_pending = -1, False
        if self.sot_probe:
            # SOT is the last token of a step of its own; what follows it is
            # fed once that step's logits are read (_sot_result)
            r.feed = prompt + self.sot[:1]
            r.chunks = self._prompt_chunks(r.feed)
            r.sot_step, r.sot_pending = len(r.chunks) - 1, True
            r.prompt_steps = len(r.chunks) + 1
        else:
            r.chunks = [r.feed[i:i + c] for i in range(0, len(r.feed), c)]
            r.prompt_steps = len(r.chunks)
        r.target = None
        text = self._window_text(r, w)
        if text is not None:
            room = self.cfg.n_text_ctx - 8 - len(prompt) - len(self.sot)
            r.target = self.tok.encode(" " + text.strip())[:room] + [self.eot]

    def _prompt_chunks(self, prompt: list[int]) -> list[list[int]]:
        """A prompt ending in SOT as step feeds of at most len(sot) tokens; SOT
        ends the last one, so no feed crosses it."""
        c = len(self.sot)
        return [prompt[i:i + c] for i in range(0, len(prompt), c)]

    def _sot_result(self, r: STTRequest, idx: int, lp: float, plp: float) -> list[int]:
        """The SOT step of ``r``'s window has retired with (language token, its
        log-probability among the candidates, log no_speech_prob): record them
        and return the host-known feed that follows SOT. Later windows of an
        utterance keep window 0's language."""
        if r.attempt > 0:
            # a fallback attempt runs the SOT step again at temperature 0: the
            # window's language and no_speech_prob are already recorded
            r.sot_pending = False
            post = [r.lang_id] + self.sot[2:]
            r.chunks.append(post)
            return post
        if r.win == 0 or r.lang_id < 0:
            r.lang_id = int(idx)
            r.language = self._lang_code.get(r.lang_id)
            r.language_prob = float(np.exp(np.float64(lp)))
            if r.language is None:
                raise RuntimeError(f"STT language detection returned token {r.lang_id}")
            counts = self.stats["languages"]
            counts[r.language] = counts.get(r.language, 0) + 1
        r.no_speech_probs.append(float(np.exp(np.float64(plp))))
        r.sot_pending = False
        post = [r.lang_id] + self.sot[2:]
        r.chunks.append(post)
        return post

    def _decode_once(self, live: list[STTRequest]) -> list[STTRequest]:
        """One decoder step over ``live`` (at most ``step_tokens`` tokens: a
        sequence may sit the step out or feed only part of its SOT prompt, see
        ``batching.plan_step``); returns the requests that finished."""
        if self._beam is not None:
            return self._beam.decode_once(live)
        take = plan_step([len(r.feed) for r in live], self.step_tokens, len(self.sot), self._rr)
        self._rr = (self._rr + self.step_tokens) % len(live) if len(live) > self.step_tokens else 0
        step, rest = [], []
        for r, n in zip(live, take):
            if n:
                step.append(r)
                rest.append(r.feed[n:])
                r.feed = r.feed[:n]
        live = step
        if self.fallback:
            nxt = self._step(live, [r.sot_pending and not x for r, x in zip(live, rest)],
                             [self._ts_ctl(r, bool(x)) for r, x in zip(live, rest)]
                             if self.timestamps or self.hotwords_on else None,
                             [self._samp(r, bool(x)) for r, x in zip(live, rest)])
        elif self.timestamps or self.hotwords_on:
            nxt = self._step(live, [r.sot_pending and not x for r, x in zip(live, rest)],
                             [self._ts_ctl(r, bool(x)) for r, x in zip(live, rest)])
        else:
            nxt = self._step(live, [r.sot_pending and not x for r, x in zip(live, rest)]) \
                if self.sot_probe else self._step(live)
        lps = plps = None
        if self.row_fields:
            nxt, lps, plps = nxt
        elif self.token_logprobs:
            nxt, lps = nxt
        self.stats["decode_steps"] += 1
        done = []
        for j, r in enumerate(live):
            if rest[j]:            # part of the prompt still to feed: logits unused
                r.feed = rest[j]
                continue
            if r.sot_pending:      # the SOT step: language and no_speech_prob
                r.feed = self._sot_result(r, int(nxt[j]), float(lps[j]), float(plps[j]))
                continue
            t = int(r.target[r.step]) if r.target is not None else int(nxt[j])
            r.tokens.append(t)
            if lps is not None and r.target is None:
                r.logprobs.append(float(lps[j]))
            r.step += 1
            if t == self.eot or len(r.tokens) >= r.max_new_tokens or \
                    (r.target is not None and r.step >= len(r.target)):
                f = self._finish(r)
                if f is not None:
                    done.append(f)
            else:
                r.feed = [t]
        return done

    def _finish(self, r: STTRequest) -> STTRequest | None:
        """Window ``r.win`` of ``r`` is decoded: start the next window (None)
        or complete the request (its windows' texts joined)."""
        toks = [x for x in r.tokens if x != self.eot]
        segs = None
        if self.timestamps and r.target is None:
            # a freely decoded window: timestamp tokens cut it into segments;
            # its text and the next window's prompt are the text tokens
            segs = cut_window(r.tokens, self.ts_begin, self.eot)
            toks = text_tokens(r.tokens, self.ts_begin, self.eot)
        self.kv.pool.free_seq(r.seq_id)
        # Whisper's no-speech rule, on a freely decoded window (a teacher-forced
        # one has no log-probabilities): its text is empty, its tokens stay out
        # of the next window's prompt and of the utterance's avg_logprob
        gated = False
        if self.no_speech and r.target is None and r.logprobs and len(r.no_speech_probs) > r.win:
            mean_lp = float(np.sum(np.asarray(r.logprobs, np.float64))) / len(r.logprobs)
            gated = r.no_speech_probs[r.win] > self.no_speech_threshold and \
                mean_lp < self.logprob_threshold
        if self.fallback:
            # temperature fallback, on a freely decoded window that the no-speech
            # rule keeps: too repetitive or too improbable and a higher
            # temperature left -> this attempt is discarded and the window decoded
            # again (the last temperature's result stays whatever its quality)
            T = self.temperatures[r.attempt]
            text = self.tok.decode(toks).strip()
            ratio = compression_ratio(text)
            if r.target is None and not gated and r.attempt + 1 < len(self.temperatures):
                mean = float(np.sum(np.asarray(r.logprobs, np.float64))) / len(r.logprobs) \
                    if r.logprobs else None
                if needs_fallback(text, mean, self.compression_ratio_threshold,
                                  self.logprob_threshold):
                    r.fallback_attempts += 1
                    self.stats["fallback_attempts"] += 1
                    r.attempt += 1
                    self._begin_window(r, r.win)
                    return None
            r.temperatures.append(T if r.target is None else 0.0)
            r.compression_ratios.append(ratio)
            if r.attempt > 0:
                self.stats["fallback_windows"] += 1
        seg_of = None
        if gated:
            r.gated_windows += 1
            self.stats["no_speech_windows"] += 1
            r.win_texts.append("")
        elif segs is not None:
            out = utterance_segments(segs, r.win, r.n_samples / 16000.0,
                                     lambda t: self.tok.decode(t, skip_from=self.ts_begin),
                                     *self._win_span(r))
            if self.align is not None:
                # per text token the index of its segment in ``r.segments``
                # (None: a segment dropped for its empty text)
                seg_of, n = [], len(r.segments)
                for sg in segs:
                    kept = bool(self.tok.decode(sg.tokens, skip_from=self.ts_begin).strip())
                    seg_of += [n if kept else None] * len(sg.tokens)
                    n += kept
            r.segments += out
            r.win_texts.append(" ".join(t for _, _, t in out))
            if segs and segs[-1].open:
                r.open_segments.append(r.win)
                self.stats["open_segments"] += 1
            self.stats["timestamp_segments"] += len(out)
            r.prev_tokens = (r.prev_tokens + toks)[-max(PREV_TOKENS, 1):]
        else:
            r.win_texts.append(self.tok.decode(toks).strip())
            r.prev_tokens = (r.prev_tokens + toks)[-max(PREV_TOKENS, 1):]
        if self.fallback and r.target is None and self.temperatures[r.attempt] > 0.5:
            r.prev_tokens = []      # Whisper's prompt reset: a hot window does not prompt the next
        if self.align is not None and not gated:
            # a kept window (not gated, not a discarded fallback attempt)
            self._align_window(r, seg_of)
        if self.hotwords_on and not gated:
            # the phrases spelled out in a kept window's text tokens, found by
            # the automaton the device walked (teacher-forced windows too, though
            # only freely decoded ones were biased)
            self.stats["hotword_windows"] += r.target is None
            if self.hw_auto is not None:
                new = [self.hw_auto.phrases[i] for i in self.hw_auto.matches(toks)]
                new = [p for p in new if p not in r.hotwords]
                r.hotwords += new
                self.stats["hotword_matches"] += len(new)
        if r.logprobs and not gated:
            # fp64 sum of the window's f32 values; -inf (nothing allowed) stays -inf
            r.lp_sum += float(np.sum(np.asarray(r.logprobs, np.float64)))
            r.lp_n += len(r.logprobs)
        if r.win + 1 < r.windows:
            self.stats["long_form_windows"] = self.stats.get("long_form_windows", 0) + 1
            r.attempt = 0
            self._begin_window(r, r.win + 1)
            return None
        r.t_done = time.perf_counter()
        r.text = " ".join(t for t in r.win_texts if t)
        if r.no_speech_probs:
            r.no_speech_prob = min(r.no_speech_probs)
        if r.segments:
            r.speech_start_s, r.speech_end_s = r.segments[0][0], r.segments[-1][1]
        if r.gated_windows and r.gated_windows == r.windows:
            self.stats["no_speech_utterances"] += 1
        if r.lp_n:
            r.avg_logprob = r.lp_sum / r.lp_n
            if np.isfinite(r.lp_sum):       # a step with nothing allowed is -inf
                self.stats["logprob_tokens"] += r.lp_n
                self.stats["logprob_sum"] += r.lp_sum
        self.stats["utterances"] += 1
        if self._live_reqs is not None:
            self._live_reqs.discard(r)
        return r

    def set_hotwords(self, phrases, boost: float | None = None) -> None:
        """Replace the hotword list (and with ``boost`` the boost) of an engine
        built with hotwords: the automaton is compiled on the host and written
        into the device buffers the captured graphs already point at, so nothing
        is captured again. An empty list makes the biasing step a no-op. Allowed
        only while no request is being decoded (``RuntimeError`` otherwise): a
        sequence's node belongs to the automaton it was advanced in."""
        from .hotwords import check_boost, compile_hotwords
        if not self.hotwords_on:
            raise ValueError("set_hotwords: the engine was built without hotwords (its steps "
                             "have no biasing launch)")
        if self._live_reqs:
            raise RuntimeError(f"set_hotwords: {len(self._live_reqs)} requests are live")
        b = self.hotword_boost if boost is None else check_boost(boost)
        auto = compile_hotwords(phrases, b, self.tok.encode, self.cfg.vocab_size)
        self.hw_table.load(auto if auto.T else None)
        self.hw_auto = auto if auto.T else None
        self.hotword_boost = b

    def align_rows(self, r: STTRequest) -> tuple[list, list, int | None, int]:
        """What the alignment of ``r``'s current window reads: (``rows``, the
        indices into ``r.tokens`` of its text tokens, the index of a sampled EOT
        or None, ``n_lead``). The row of sampled token k is the input position
        whose logits produced it, ``prompt_len - 1 + k``; ``rows`` = the
        positions of the SOT-sequence inputs but the last (``n_lead`` leading
        rows: normalised over, then dropped), the text tokens' rows, the EOT's.
        Rows that produced timestamp tokens and the previous-text prompt are
        left out."""
        ts_begin = self.ts_begin if self.timestamps else None
        idx = [k for k, t in enumerate(r.tokens)
               if t != self.eot and (ts_begin is None or t < ts_begin)]
        eot_k = next((k for k, t in enumerate(r.tokens) if t == self.eot), None)
        n_lead = len(self.sot) - 1
        p0, base = r.prompt_len - len(self.sot), r.prompt_len - 1
        rows = list(range(p0, p0 + n_lead)) + [base + k for k in idx]
        if eot_k is not None:
            rows.append(base + eot_k)
        return rows, idx, eot_k, n_lead

    def window_frames(self, r: STTRequest) -> int:
        """20 ms frames of the audio in ``r``'s current window."""
        if r.win_frames is not None:
            a, b = r.win_frames[r.win]
            return ops.ref.align_frames(min(b * 320, r.n_samples) - a * 320, self.cfg.n_audio_ctx)
        return ops.ref.align_frames(min(N_SAMPLES, r.n_samples - r.win * N_SAMPLES),
                                    self.cfg.n_audio_ctx)

    @staticmethod
    def _win_span(r: STTRequest) -> tuple:
        """(start, end) of ``r``'s current window in utterance seconds, as
        ``utterance_segments`` / ``utterance_words`` take them: ``win_starts``
        and, for a planned window, its end (None: the utterance's duration
        bounds it, as for the fixed 30 s windows)."""
        off = r.win_starts[r.win] if r.win < len(r.win_starts) else None
        end = r.win_frames[r.win][1] / 50 if r.win_frames is not None else None
        return off, end

    def _align_window(self, r: STTRequest, seg_of: list | None) -> None:
        """Word timestamps of ``r``'s kept window: three launches on this
        stream (scores, cost, DTW) over the queries its steps recorded, one
        synchronous read-back of ``tok_frame``, then the host's word assembly.
        Writes to the query store go by (slot, position) and are stream-ordered
        before this: a fallback retry, a discarded speculative step or a reused
        slot only touched positions outside ``rows`` or rewrote them since."""
        rows, idx, eot_k, n_lead = self.align_rows(r)
        if not idx:
            r.token_frames.append([])
            return
        F = self.window_frames(r)
        frames = self.align.align(r.slot, rows, self.xkv, F, n_lead)
        r.token_frames.append(frames)
        lps = [r.logprobs[k] for k in idx] \
            if r.target is None and len(r.logprobs) == len(r.tokens) else None
        if seg_of is None:
            seg_of = [r.win] * len(idx)
        words = window_words(self.tok.decode, [r.tokens[k] for k in idx], frames[: len(idx)],
                             frames[len(idx)] if eot_k is not None else F, lps,
                             r.language or self.language, seg_of)
        r.words += utterance_words(words, r.win, r.n_samples / 16000.0, *self._win_span(r))
        r.word_segments += [w.segment for w in words]
        self.stats["aligned_windows"] += 1
        self.stats["aligned_words"] += len(words)

    def transcribe(self, reqs: list[STTRequest], device_pcm: torch.Tensor | None = None
                   ) -> list[STTRequest]:
        """Synchronous batch: encode all, decode until every request is done."""
        if not reqs:
            return reqs
        rows = self.rows_needed(reqs)
        assert rows <= self.max_slots, "batch (30 s windows) exceeds max_batch"
        self._admit(reqs, list(range(rows)), device_pcm)
        self._spare_slots.clear()       # no scheduler: the slots were this call's own
        t_dec = time.monotonic()
        live, steps = [r for r in reqs if r.t_done == 0.0], 0
        while live:
            self._decode_once(live)
            steps += 1
            live = [r for r in live if r.t_done == 0.0]
        tracer().record("stt_decode", t_dec, time.monotonic(), steps=steps, batch=len(reqs))
        return reqs

    # --------------------------------------------- continuous batching
    def start(self, stream_priority: int = 0) -> None:
        """Start the STT scheduler thread: requests submitted with
        ``submit_batch`` are encoded on arrival and join the RUNNING decoder
        batch at the next step boundary (each in its own cross-attention slot),
        so an utterance never waits for an earlier batch's decode to drain."""
        if getattr(self, "_sched", None) is not None:
            return
        from ..utils.gil import tune_switch_interval
        tune_switch_interval()
        self._inbox: queue.Queue = queue.Queue()
        self._running = True
        self._free_slots = list(range(self.max_slots))
        self._sched = threading.Thread(target=self._schedule, args=(stream_priority,),
                                       name="stt-scheduler", daemon=True)
        self._sched.start()

    def stop(self) -> None:
        if getattr(self, "_sched", None) is None:
            return
        self._running = False
        self._inbox.put(None)
        self._sched.join(timeout=60)
        self._sched = None

    def submit_batch(self, reqs: list[STTRequest], on_done=None) -> Future:
        """Queue requests; ``on_done(req)`` fires on the scheduler thread as
        each finishes; the future resolves with ``reqs`` when all are done."""
        self.start()
        fut: Future = Future()
        if getattr(self, "_fatal", None) is not None:
            fut.set_exception(self._fatal)
            return fut
        reqs = list(reqs)
        if len(reqs) > 1 and self.rows_needed(reqs) > self.max_slots:
            # admission needs a free slot for every window of an inbox item: an
            # oversize batch would wait forever, so it goes in smaller items
            return join_futures([self.submit_batch([r], on_done) for r in reqs], reqs)
        if self.rows_needed(reqs) > self.max_slots:
            fut.set_exception(ValueError(f"utterance needs {self.rows_needed(reqs)} 30 s windows "
                                         f"> max_batch {self.max_slots}"))
            return fut
        self._inbox.put((reqs, on_done, fut))
        return fut

    def _schedule(self, stream_priority: int) -> None:
        try:
            if self.is_gpu:
                from ..utils.streams import placed_stream
                torch.cuda.set_device(self.device)
                torch.cuda.set_stream(placed_stream(self.device, "stt", stream_priority))
                if os.environ.get("LOQA_STT_WAVE_PRIO", "0") == "1":
                    # the latency-bound decoder's waves win issue arbitration
                    # against co-resident LLM GEMM waves (set per thread)
                    ops.set_launch_priority(1)
        except Exception as e:  # noqa: BLE001 - never leave submitters waiting
            self._fatal = e
            while True:
                try:
                    it = self._inbox.get_nowait()
                except queue.Empty:
                    return
                if it is not None and not it[2].done():
                    it[2].set_exception(e)
        live: list[STTRequest] = []
        waiting: list[tuple] = []          # (reqs, cb, fut) not yet admitted (no free slot)
        encoding: list[tuple] = []         # (reqs, future) on the encoder worker
        cells: dict[int, list] = {}
        head_bypass = 0                     # admissions that passed the blocked head
        # the encoder runs on its own worker thread + stream, overlapped with
        # the running decoder batch (an arrival's encode no longer stalls every
        # live transcription); requests join at the next step boundary after
        # their encoder output and cross-attention K|V are complete (inline
        # encodes measured 1.8x slower, docs/PERF.md)
        overlap = self.is_gpu
        enc_pool = self._encoder_executor() if overlap else None
        pl = None
        if self.pipelined:
            from .stt_pipeline import STTPipeline
            pl = STTPipeline(self)
        while self._running:
            idle = not live and not waiting and not encoding
            items = [self._inbox.get()] if idle else []
            while True:
                try:
                    items.append(self._inbox.get_nowait())
                except queue.Empty:
                    break
            for it in items:
                if it is not None:
                    waiting.append(it)
            try:
                new: list[STTRequest] = []
                quiet: list[STTRequest] = []      # VAD-silent: finished at admission
                n_rows = 0
                self._reclaim_spare()
                # FIFO, except that items which fit may pass a head that does
                # not (a long-form utterance waiting for many free slots), at
                # most HOL_BYPASS times per head so it is never starved
                i = 0
                while i < len(waiting):
                    need = self.rows_needed(waiting[i][0])
                    if need > len(self._free_slots) - n_rows:
                        if i == 0 and head_bypass < HOL_BYPASS:
                            i = 1
                            continue
                        if i == 0:
                            break
                        i += 1
                        continue
                    reqs, cb, fut = waiting.pop(i)
                    if i == 0:
                        head_bypass = 0
                    else:
                        head_bypass += 1
                        self.stats["hol_bypass"] = self.stats.get("hol_bypass", 0) + 1
                        if head_bypass >= HOL_BYPASS:
                            i = len(waiting)      # the head goes next
                    n_rows += need
                    if not reqs:
                        fut.set_result(reqs)
                        continue
                    cell = [len(reqs), fut, reqs, cb]
                    cells[id(cell)] = cell
                    for r in reqs:
                        r.on_done = cell
                    new += reqs
                if new:
                    slots = [self._free_slots.pop(0) for _ in range(n_rows)]
                    if enc_pool is not None:
                        encoding.append((new, enc_pool.submit(self._encode, new, slots)))
                    else:
                        self._admit(new, slots)
                        self._reclaim_spare()
                        quiet += [r for r in new if r.t_done != 0.0]
                        new = [r for r in new if r.t_done == 0.0]
                        if pl is not None:
                            for r in new:
                                pl.admit(r)
                        live += new
                if encoding:
                    if not live:
                        wait([f for _, f in encoding], timeout=0.002, return_when=FIRST_COMPLETED)
                    still = []
                    for reqs, f in encoding:
                        if f.done():
                            f.result()
                            self._start_decode(reqs)
                            self._reclaim_spare()
                            quiet += [r for r in reqs if r.t_done != 0.0]
                            reqs = [r for r in reqs if r.t_done == 0.0]
                            if pl is not None:
                                for r in reqs:
                                    pl.admit(r)
                            live += reqs
                        else:
                            still.append((reqs, f))
                    encoding = still
                if live or quiet:
                    finished = quiet
                    if live:
                        finished = quiet + (pl.pump(live) if pl is not None
                                            else self._decode_once(live))
                    for r in finished:
                        self._free_slots += [] if r.vad_silent else r.slots or [r.slot]
                        self._free_slots.sort()
                        cell = r.on_done
                        if cell[3] is not None:
                            cell[3](r)
                        cell[0] -= 1
                        if cell[0] == 0:
                            cells.pop(id(cell), None)
                            cell[1].set_result(cell[2])
                    live = [r for r in live if r.t_done == 0.0]
            except Exception as e:  # noqa: BLE001 - fail every waiting batch loudly
                # encoder jobs already submitted keep writing cross-attention K|V
                # into their slots: let them finish before any slot is reused
                wait([f for _, f in encoding])
                if pl is not None:
                    pl.abort()
                for cell in list(cells.values()):
                    if not cell[1].done():
                        cell[1].set_exception(e)
                for r in live:
                    if self._beam is not None:
                        self._beam.abort(r)
                    self.kv.pool.free_seq(r.seq_id)
                for _, _, fut in waiting:
                    if not fut.done():
                        fut.set_exception(e)
                live, waiting, cells, encoding = [], [], {}, []
                if self._live_reqs is not None:
                    self._live_reqs.clear()
                self._spare_slots.clear()
                self._free_slots = list(range(self.max_slots))

    def _encoder_executor(self) -> ThreadPoolExecutor:
        if getattr(self, "_enc_pool", None) is None:
            dev = self.device

            def init():
                from ..utils.streams import placed_stream
                torch.cuda.set_device(dev)
                torch.cuda.set_stream(placed_stream(dev, "encoder"))
            self._enc_pool = ThreadPoolExecutor(1, thread_name_prefix="stt-encoder", initializer=init)
        return self._enc_pool

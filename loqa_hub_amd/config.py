"""Typed configuration loaded from the environment.

Same variable names and defaults as the reference (``internal/config/config.go``:
Load :113-174, validate :177-211; helpers :214-255 silently fall back to the
default on a parse error). Differences, all additive:

* ONE config object: ``OLLAMA_URL``/``OLLAMA_MODEL``, ``NATS_URL``, ``DB_PATH``
  and ``LOG_*`` are read here instead of ad hoc in each component;
* documented aliases are accepted (``LOQA_HUB_PORT``, ``DB_PATH``,
  ``STREAMING_VISUAL_FEEDBACK_DELAY``, ``ARBITRATION_WINDOW_DURATION``,
  ``MAX_CONCURRENT_RELAYS``) - the reference's own names win when both are set;
* GPU keys for the on-device pipeline (``HUB_*``) and arbitration scope.

Durations use Go syntax (``300ms``, ``1h30m``, ``2s``).
"""
from __future__ import annotations

import math
import os
import re
from dataclasses import dataclass, field

# PCM sample rates the hub converts between (csrc/kernels/resample.hip): what a
# relay may record at (HUB_AUDIO_INPUT_RATE=relay) and a reply may be played at
# (HUB_TTS_SAMPLE_RATE)
AUDIO_SAMPLE_RATES = (8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000)
# the frame sizes (samples) the FLAC encoder of the gpu voice offers (HUB_TTS_FLAC_BLOCK)
FLAC_BLOCK_SIZES = (256, 512, 1024, 2048, 4096)

# limits of the STT hotword list (engine/hotwords.py): phrases, and tokens per
# token variant of a phrase. ``validate`` holds the list to the first; the
# second needs the STT tokenizer (``GPUConfig.check_hotwords``, and again when the
# engine compiles the list at start-up)
HOTWORD_MAX_PHRASES = 1024
HOTWORD_MAX_TOKENS = 16

# VadConfig field -> the knob that sets it (Config.validate names the knob)
_VAD_KEYS = {"threshold_db": "HUB_VAD_THRESHOLD_DB", "min_level_dbfs": "HUB_VAD_MIN_LEVEL_DBFS",
             "floor_max_dbfs": "HUB_VAD_FLOOR_MAX_DBFS", "floor_s": "HUB_VAD_FLOOR_S",
             "min_speech_ms": "HUB_VAD_MIN_SPEECH_MS", "min_silence_ms": "HUB_VAD_MIN_SILENCE_MS",
             "pad_ms": "HUB_VAD_PAD_MS"}

_DUR_RE = re.compile(r"([0-9]*\.?[0-9]+)(ns|us|µs|ms|s|m|h)")
_UNIT = {"ns": 1e-9, "us": 1e-6, "µs": 1e-6, "ms": 1e-3, "s": 1.0, "m": 60.0, "h": 3600.0}


def parse_go_duration(s: str) -> float:
    """Go time.ParseDuration subset -> seconds. Raises ValueError."""
    s = s.strip()
    if s in ("0", "+0", "-0"):
        return 0.0
    sign = 1.0
    if s[:1] in "+-":
        sign = -1.0 if s[0] == "-" else 1.0
        s = s[1:]
    if not s:
        raise ValueError("empty duration")
    pos, total = 0, 0.0
    for m in _DUR_RE.finditer(s):
        if m.start() != pos:
            raise ValueError(f"invalid duration {s!r}")
        total += float(m.group(1)) * _UNIT[m.group(2)]
        pos = m.end()
    if pos != len(s):
        raise ValueError(f"invalid duration {s!r}")
    return sign * total


def format_go_duration(sec: float) -> str:
    if sec == 0:
        return "0s"
    if abs(sec) < 1:
        ms = sec * 1e3
        return f"{ms:g}ms"
    h, rem = divmod(sec, 3600)
    m, s = divmod(rem, 60)
    out = ""
    if h:
        out += f"{int(h)}h"
    if h or m:
        out += f"{int(m)}m"
    return out + f"{s:g}s"


def _get(env, *keys):
    for k in keys:
        v = env.get(k, "")
        if v != "":
            return v
    return ""


def env_str(env, default: str, *keys) -> str:
    v = _get(env, *keys)
    return v if v != "" else default


_INT_RE = re.compile(r"^[+-]?[0-9]+$")


def env_int(env, default: int, *keys) -> int:
    v = _get(env, *keys)
    return int(v, 10) if _INT_RE.match(v) else default


def env_float(env, default: float, *keys) -> float:
    v = _get(env, *keys)
    try:
        return float(v) if v != "" else default
    except ValueError:
        return default


_TRUE = {"1", "t", "T", "true", "TRUE", "True"}
_FALSE = {"0", "f", "F", "false", "FALSE", "False"}


def env_bool(env, default: bool, *keys) -> bool:
    v = _get(env, *keys)
    if v in _TRUE:
        return True
    if v in _FALSE:
        return False
    return default


def env_duration(env, default: float, *keys) -> float:
    v = _get(env, *keys)
    try:
        return parse_go_duration(v) if v != "" else default
    except ValueError:
        return default


@dataclass
class ServerConfig:
    host: str = "0.0.0.0"
    port: int = 8080
    grpc_port: int = 50051
    db_path: str = "./data/loqa-hub.db"
    read_timeout: float = 30.0
    write_timeout: float = 30.0


@dataclass
class STTConfig:
    url: str = "http://stt:8000"
    language: str = "en"
    temperature: float = 0.0
    max_tokens: int = 224


@dataclass
class TTSConfig:
    url: str = "http://localhost:8880/v1"
    voice: str = "af_bella"
    speed: float = 1.0
    response_format: str = "wav"
    normalize: bool = True
    max_concurrent: int = 10
    timeout: float = 10.0
    fallback_enabled: bool = True


@dataclass
class StreamingConfig:
    enabled: bool = False
    ollama_url: str = "http://ollama:11434"
    model: str = "llama3.2:3b"
    max_buffer_time: float = 2.0
    max_tokens_per_phrase: int = 50
    audio_concurrency: int = 3
    visual_feedback_delay: float = 0.050
    interrupt_timeout: float = 0.500
    fallback_enabled: bool = True
    metrics_enabled: bool = True


@dataclass
class LoggingConfig:
    level: str = "info"
    format: str = "json"


@dataclass
class NATSConfig:
    url: str = "nats://localhost:4222"
    subject: str = "loqa.commands"
    max_reconnect: int = 10
    reconnect_wait: float = 2.0


@dataclass
class PrivacyConfig:
    data_retention: float = 30 * 24 * 3600.0
    zero_persistence: bool = False
    auto_cleanup_enabled: bool = True
    cleanup_interval: float = 24 * 3600.0


@dataclass
class OllamaConfig:
    """The service-level parser endpoint (reference: env-only in
    audio_service.go:204-212; default http://localhost:11434)."""
    url: str = "http://localhost:11434"
    model: str = "llama3.2:3b"


@dataclass
class GPUConfig:
    """On-device pipeline (SURVEY §5.6 'New')."""
    num_gpus: int = 0                 # 0 = all visible
    dp: int = 0                       # 0 = num_gpus
    tp: int = 1
    stt_model: str = "whisper-base"
    llm_model: str = "tinyllama"
    tts_model: str = "vits-ljs"
    dtype: str = "bf16"
    max_batch: int = 64
    kv_block: int = 16
    max_seq_len: int = 1024
    llm_backend: str = "gpu"          # gpu | ollama
    # LLM projection / lm_head weights: bf16, fp8 (e4m3 weight streams with
    # per-row scales: half the bytes per decode step; one GPU, gpu backend) or
    # mxfp4 (projections as e2m1 with a power-of-two scale per 32 weights, 4.25
    # bits per weight, the lm_head as fp8; one GPU, gpu backend)
    llm_weights: str = "bf16"
    stt_backend: str = "gpu"          # gpu | http
    # the transcript's confidence: "heuristic" (the reference's text rules) or
    # "acoustic" (exp of the mean log-probability of the Whisper tokens; gpu
    # backend); below stt_confirm_below the hub asks the user to confirm
    stt_confidence: str = "heuristic"
    stt_confirm_below: float = 0.6
    # STT_LANGUAGE=auto (or set and empty): candidate languages of the gpu
    # backend's detection ([] = every language the tokenizer has)
    stt_languages: list = field(default_factory=list)
    # Whisper's no-speech rule on the gpu backend: a 30 s window whose
    # no_speech_prob > stt_no_speech_threshold and whose mean token
    # log-probability < stt_logprob_threshold gives no text (the reference's
    # STT service answers such a segment with an empty transcript)
    stt_no_speech: str = "off"        # off | on
    stt_no_speech_threshold: float = 0.6
    stt_logprob_threshold: float = -1.0
    # Whisper's default decoding mode on the gpu backend: "segment" drops
    # <|notimestamps|> from the prompt, samples under the timestamp rules and
    # reports (start, end, text) segments; a window's first timestamp is at
    # most stt_max_initial_timestamp seconds
    stt_timestamps: str = "off"       # off | segment
    stt_max_initial_timestamp: float = 1.0
    # Whisper's temperature fallback on the gpu backend: a 30 s window whose
    # text compresses better than stt_compression_ratio_threshold (a repetition
    # loop) or whose mean token log-probability is below stt_logprob_threshold
    # is decoded again at the next temperature of the list, sampled on the
    # device; [0.0] = off (greedy only)
    stt_temperature: list = field(default_factory=lambda: [0.0])
    stt_compression_ratio_threshold: float = 2.4
    # word timestamps on the gpu backend (with or without stt_timestamps): the
    # decoder keeps the cross-attention queries of the alignment heads and every
    # kept 30 s window is aligned on the device (dynamic time warping);
    # stt_alignment_heads = "layer:head,..." (at most 32; empty: the checkpoint's
    # generation config, else every head of the upper half of the decoder layers)
    stt_word_timestamps: str = "off"  # off | on
    stt_alignment_heads: str = ""
    # beam search on the gpu backend (Whisper's BeamSearchDecoder, patience 1):
    # hypotheses per freely decoded 30 s window, 1 = off (greedy). Not together
    # with stt_timestamps, stt_word_timestamps or a temperature fallback list.
    stt_beam_size: int = 1
    # hotword biasing on the gpu backend: phrases (device, room and product
    # names) whose tokens get stt_hotword_boost added to their logit, once per
    # decoder step, while the decoded text is inside one of them (an
    # Aho-Corasick automaton matched on the device). stt_hotwords holds
    # HUB_STT_HOTWORDS merged with the lines of stt_hotwords_file;
    # stt_hotwords_skills = on adds the keywords of the loaded skill manifests
    # at start-up. The boost is in logit units and may be negative; its default
    # is the context-score convention of shallow-fusion biasing, not a measured
    # optimum. Not together with stt_beam_size > 1.
    stt_hotwords: list = field(default_factory=list)
    stt_hotwords_file: str = ""
    stt_hotword_boost: float = 2.0
    stt_hotwords_skills: str = "off"  # off | on
    # voice activity detection on the gpu backend, over the relay PCM the ingest
    # path holds on the device: an utterance without speech is answered with
    # no_speech before any encoder pass, the encoder windows start and end at
    # speech and long audio is cut at pauses instead of fixed 30 s marks. A 20 ms
    # frame is speech when its mean square is at least vad_min_level_dbfs and
    # vad_threshold_db above the noise floor (the minimum within vad_floor_s on
    # each side, at most vad_floor_max_dbfs); runs shorter than
    # vad_min_speech_ms are dropped, gaps shorter than vad_min_silence_ms filled,
    # vad_pad_ms added around speech (milliseconds: multiples of 20). The
    # defaults are not tuned on speech data; they lean towards keeping audio.
    stt_vad: str = "off"              # off | on
    vad_threshold_db: float = 9.0
    vad_min_level_dbfs: float = -55.0
    vad_floor_max_dbfs: float = -30.0
    vad_floor_s: float = 3.0
    vad_min_speech_ms: int = 100
    vad_min_silence_ms: int = 500
    vad_pad_ms: int = 200
    # relay audio: "fixed" (every chunk is 16 kHz, AudioChunk.sample_rate is
    # ignored: the reference's behaviour) or "relay" (the stream's own rate, one
    # of AUDIO_SAMPLE_RATES; the gpu STT resamples it to 16 kHz on the device,
    # an external STT gets it in the WAV header)
    audio_input_rate: str = "fixed"
    # reply audio of the gpu voice: 0 = the voice's own rate (22.05 kHz random
    # init, 16 kHz MMS), else one of AUDIO_SAMPLE_RATES (resampled on the device)
    tts_sample_rate: int = 0
    tts_backend: str = "gpu"          # gpu | http | none
    use_graphs: bool = True
    seed: int = 0
    tp_fallback_model: str = "llama3-8b"   # a failed TP group degrades to this ("none": off)
    # the fallback's weights (+ tokenizer in / beside it); required when
    # llm_checkpoint is set (no silent swap to a random-init model)
    tp_fallback_checkpoint: str = ""
    stt_checkpoint: str = ""          # safetensors file/dir (HF naming); "" = seeded random init
    llm_checkpoint: str = ""
    tts_checkpoint: str = ""          # HF VITS / MMS-TTS dir; "" = the random-init HUB_TTS_MODEL
    # what a TTS_FORMAT the GPU voice cannot encode (mp3, opus, aac) gets:
    # "wav" = WAV, labelled wav, logged + counted; "error" = the synthesis fails.
    # wav, pcm and flac are encoded (flac on the device, csrc/kernels/flac.hip)
    tts_format_policy: str = "wav"
    # samples per frame of a flac reply, one of FLAC_BLOCK_SIZES (docs/PERF.md
    # "FLAC replies" has the measurement behind the default)
    tts_flac_block: int = 4096
    # tokenizer.json of a checkpoint ("": the one in / beside the checkpoint;
    # no checkpoint: the synthetic tokenizer of the random-init weights)
    stt_tokenizer: str = ""
    llm_tokenizer: str = ""

    def llm_config(self):
        """The intent model's shape: the checkpoint's own config.json when it
        has one (any Llama-family checkpoint), else the named ``HUB_LLM_MODEL``."""
        from .models.configs import checkpoint_config, llama_config, llama_config_from_hf
        d = checkpoint_config(self.llm_checkpoint)
        return llama_config_from_hf(d, self.llm_model) if d else llama_config(self.llm_model)

    def tp_fallback_config(self):
        """Shape of the TP failover engine: its checkpoint's config.json, else
        ``HUB_TP_FALLBACK_MODEL``."""
        from .models.configs import checkpoint_config, llama_config, llama_config_from_hf
        d = checkpoint_config(self.tp_fallback_checkpoint)
        return llama_config_from_hf(d, self.tp_fallback_model) if d else \
            llama_config(self.tp_fallback_model)

    def stt_config(self):
        """As ``llm_config`` for the Whisper checkpoint / ``HUB_STT_MODEL``."""
        from .models.configs import checkpoint_config, whisper_config, whisper_config_from_hf
        d = checkpoint_config(self.stt_checkpoint)
        return whisper_config_from_hf(d, self.stt_model) if d else whisper_config(self.stt_model)

    def tokenizer(self, which: str, vocab_size: int):
        """The tokenizer for ``which`` ("stt" / "llm"): an explicit
        ``HUB_*_TOKENIZER``, else the checkpoint's own file, else None."""
        from .engine.tokenizer import find_tokenizer, load_tokenizer
        explicit = getattr(self, f"{which}_tokenizer")
        if explicit:
            return load_tokenizer(explicit, vocab_size)
        ckpt = getattr(self, f"{which}_checkpoint")
        return load_tokenizer(ckpt, vocab_size) if find_tokenizer(ckpt) else None

    def vad_config(self, always: bool = False):
        """``VadConfig`` of the ``HUB_VAD_*`` knobs for ``STTEngine(vad=...)``
        (None: ``HUB_STT_VAD=off``, unless ``always``); ValueError for a value
        out of range."""
        if self.stt_vad != "on" and not always:
            return None
        from .engine.stt_vad import VadConfig
        return VadConfig(self.vad_threshold_db, self.vad_min_level_dbfs, self.vad_floor_max_dbfs,
                         self.vad_floor_s, self.vad_min_speech_ms, self.vad_min_silence_ms,
                         self.vad_pad_ms)

    @property
    def hotwords_on(self) -> bool:
        """Hotword biasing is configured (a phrase list or the skills source)."""
        return bool(self.stt_hotwords) or self.stt_hotwords_skills == "on"

    def resolve_hotwords(self, manifests=()) -> list:
        """The one plain list every STT engine of the hub gets: stt_hotwords,
        then (stt_hotwords_skills = on) the ``keywords`` of ``manifests`` in
        order; phrases normalised, duplicates collapsed, held to the phrase
        limit."""
        out = list(self.stt_hotwords)
        if self.stt_hotwords_skills == "on":
            for m in manifests:
                out += [str(k) for k in (getattr(m, "keywords", None) or [])]
        out = _hotword_list(out)
        if len(out) > HOTWORD_MAX_PHRASES:
            raise ConfigError(f"invalid configuration: {len(out)} STT hotwords (HUB_STT_HOTWORDS, "
                              "HUB_STT_HOTWORDS_FILE and skill keywords) exceed the limit of "
                              f"{HOTWORD_MAX_PHRASES}: {out[HOTWORD_MAX_PHRASES]!r}")
        return out

    def check_hotwords(self, phrases, encode=None, vocab_size: int | None = None) -> None:
        """``phrases`` against the limits that need the STT tokenizer (tokens per
        variant, token ids within the vocabulary, the table's capacity); the
        hub's start-up calls it on the resolved list. ``encode`` / ``vocab_size``
        default to the configured STT model's tokenizer."""
        from .engine.hotwords import compile_hotwords
        if encode is None:
            from .engine.tokenizer import get_tokenizer
            vocab_size = self.stt_config().vocab_size
            encode = (self.tokenizer("stt", vocab_size) or get_tokenizer(vocab_size)).encode
        try:
            compile_hotwords(phrases, self.stt_hotword_boost, encode, vocab_size)
        except ValueError as e:
            raise ConfigError(f"invalid configuration: HUB_STT_HOTWORDS: {e}") from None


@dataclass
class ArbitrationConfig:
    window: float = 0.300
    scope: str = "global"             # global | per_relay_group
    max_concurrent_relays: int = 0    # 0 = unlimited
    end_of_speech_wait: float = 5.0
    bridge_timeout: float = 2.0
    confirmation_enabled: bool = False
    relay_groups: dict = field(default_factory=dict)  # relay id -> room/group
    # per_relay_group scope: a relay whose group (static ARBITRATION_RELAY_GROUPS
    # map) has no other member cannot collide, so it wins at once instead of
    # waiting out the window ("Single relay: No additional latency (bypass
    # arbitration)", reference docs/COLLISION_DETECTION.md:203; the reference's
    # code always waits, audio_service.go:443,494-502, hence opt-in)
    single_relay_bypass: bool = False


@dataclass
class Config:
    server: ServerConfig = field(default_factory=ServerConfig)
    stt: STTConfig = field(default_factory=STTConfig)
    tts: TTSConfig = field(default_factory=TTSConfig)
    streaming: StreamingConfig = field(default_factory=StreamingConfig)
    logging: LoggingConfig = field(default_factory=LoggingConfig)
    nats: NATSConfig = field(default_factory=NATSConfig)
    privacy: PrivacyConfig = field(default_factory=PrivacyConfig)
    ollama: OllamaConfig = field(default_factory=OllamaConfig)
    gpu: GPUConfig = field(default_factory=GPUConfig)
    arbitration: ArbitrationConfig = field(default_factory=ArbitrationConfig)

    def validate(self) -> None:
        if self.server.port <= 0 or self.server.port > 65535:
            raise ConfigError(f"invalid server port: {self.server.port}")
        if self.server.grpc_port <= 0 or self.server.grpc_port > 65535:
            raise ConfigError(f"invalid gRPC port: {self.server.grpc_port}")
        if self.stt.url == "":
            raise ConfigError("STT URL must be provided")
        if self.tts.url == "":
            raise ConfigError("TTS URL must be provided")
        if self.tts.max_concurrent <= 0:
            raise ConfigError(f"TTS max concurrent must be positive: {self.tts.max_concurrent}")
        if self.tts.speed <= 0:
            raise ConfigError(f"TTS speed must be positive: {self.tts.speed:f}")
        if self.privacy.data_retention < 0:
            raise ConfigError("data retention duration cannot be negative: "
                              f"{format_go_duration(self.privacy.data_retention)}")
        if self.privacy.cleanup_interval <= 0:
            raise ConfigError("cleanup interval must be positive: "
                              f"{format_go_duration(self.privacy.cleanup_interval)}")
        if self.arbitration.scope not in ("global", "per_relay_group"):
            raise ConfigError(f"invalid ARBITRATION_SCOPE: {self.arbitration.scope}")
        if self.gpu.tp < 1:
            raise ConfigError(f"HUB_TP must be >= 1: {self.gpu.tp}")
        if self.gpu.llm_weights not in ("bf16", "fp8", "mxfp4"):
            raise ConfigError(f"invalid HUB_LLM_WEIGHTS (bf16 | fp8 | mxfp4): {self.gpu.llm_weights}")
        if self.gpu.llm_weights != "bf16":
            wd = self.gpu.llm_weights
            if self.gpu.tp > 1:
                raise ConfigError(f"HUB_LLM_WEIGHTS={wd} needs HUB_TP=1 (no tensor-parallel {wd} "
                                  f"shards): HUB_TP={self.gpu.tp}")
            if self.gpu.llm_backend != "gpu":
                raise ConfigError(f"HUB_LLM_WEIGHTS={wd} needs HUB_LLM_BACKEND=gpu: "
                                  f"{self.gpu.llm_backend}")
        if self.gpu.stt_confidence not in ("heuristic", "acoustic"):
            raise ConfigError("invalid HUB_STT_CONFIDENCE (heuristic | acoustic): "
                              f"{self.gpu.stt_confidence}")
        if self.gpu.stt_confidence == "acoustic" and self.gpu.stt_backend != "gpu":
            raise ConfigError("HUB_STT_CONFIDENCE=acoustic needs HUB_STT_BACKEND=gpu: "
                              f"{self.gpu.stt_backend}")
        if self.gpu.audio_input_rate not in ("fixed", "relay"):
            raise ConfigError("invalid HUB_AUDIO_INPUT_RATE (fixed | relay): "
                              f"{self.gpu.audio_input_rate}")
        if self.gpu.tts_sample_rate != 0 and self.gpu.tts_sample_rate not in AUDIO_SAMPLE_RATES:
            raise ConfigError("invalid HUB_TTS_SAMPLE_RATE (0 | "
                              f"{' | '.join(map(str, AUDIO_SAMPLE_RATES))}): "
                              f"{self.gpu.tts_sample_rate}")
        if self.gpu.tts_flac_block not in FLAC_BLOCK_SIZES:
            raise ConfigError("invalid HUB_TTS_FLAC_BLOCK ("
                              f"{' | '.join(map(str, FLAC_BLOCK_SIZES))}): "
                              f"{self.gpu.tts_flac_block}")
        if not 0.0 <= self.gpu.stt_confirm_below <= 1.0:
            raise ConfigError("HUB_STT_CONFIRM_BELOW must be in [0, 1]: "
                              f"{self.gpu.stt_confirm_below}")
        if self.gpu.stt_no_speech not in ("off", "on"):
            raise ConfigError(f"invalid HUB_STT_NO_SPEECH (off | on): {self.gpu.stt_no_speech}")
        if self.gpu.stt_no_speech == "on" and self.gpu.stt_backend != "gpu":
            raise ConfigError("HUB_STT_NO_SPEECH=on needs HUB_STT_BACKEND=gpu: "
                              f"{self.gpu.stt_backend}")
        if not 0.0 < self.gpu.stt_no_speech_threshold <= 1.0:
            raise ConfigError("HUB_STT_NO_SPEECH_THRESHOLD must be in (0, 1]: "
                              f"{self.gpu.stt_no_speech_threshold}")
        if not self.gpu.stt_logprob_threshold <= 0.0:
            raise ConfigError("HUB_STT_LOGPROB_THRESHOLD must be <= 0: "
                              f"{self.gpu.stt_logprob_threshold}")
        if self.gpu.stt_timestamps not in ("off", "segment"):
            raise ConfigError("invalid HUB_STT_TIMESTAMPS (off | segment): "
                              f"{self.gpu.stt_timestamps}")
        if self.gpu.stt_timestamps == "segment" and self.gpu.stt_backend != "gpu":
            raise ConfigError("HUB_STT_TIMESTAMPS=segment needs HUB_STT_BACKEND=gpu: "
                              f"{self.gpu.stt_backend}")
        if self.gpu.stt_word_timestamps not in ("off", "on"):
            raise ConfigError("invalid HUB_STT_WORD_TIMESTAMPS (off | on): "
                              f"{self.gpu.stt_word_timestamps}")
        if self.gpu.stt_word_timestamps == "on" and self.gpu.stt_backend != "gpu":
            raise ConfigError("HUB_STT_WORD_TIMESTAMPS=on needs HUB_STT_BACKEND=gpu: "
                              f"{self.gpu.stt_backend}")
        if self.gpu.stt_alignment_heads:
            if not re.fullmatch(r"\d+:\d+(,\d+:\d+){0,31}", self.gpu.stt_alignment_heads):
                raise ConfigError("HUB_STT_ALIGNMENT_HEADS must be 'layer:head,...' (at most 32): "
                                  f"{self.gpu.stt_alignment_heads}")
        if not 0.0 <= self.gpu.stt_max_initial_timestamp <= 30.0:
            raise ConfigError("HUB_STT_MAX_INITIAL_TIMESTAMP must be in [0, 30] seconds: "
                              f"{self.gpu.stt_max_initial_timestamp}")
        t = self.gpu.stt_temperature
        if not t or t[0] != 0.0 or any(not 0.0 <= x <= 1.0 for x in t) or \
                any(b <= a for a, b in zip(t, t[1:])):
            raise ConfigError("HUB_STT_TEMPERATURE must be a strictly increasing list within "
                              f"[0, 1] that starts at 0: {t}")
        if len(t) > 1 and self.gpu.stt_backend != "gpu":
            raise ConfigError("HUB_STT_TEMPERATURE with a fallback needs HUB_STT_BACKEND=gpu: "
                              f"{self.gpu.stt_backend}")
        b = self.gpu.stt_beam_size
        if not 1 <= b <= 8:
            raise ConfigError(f"HUB_STT_BEAM_SIZE must be in 1..8: {b}")
        if b > 1:
            if self.gpu.stt_backend != "gpu":
                raise ConfigError("HUB_STT_BEAM_SIZE > 1 needs HUB_STT_BACKEND=gpu: "
                                  f"{self.gpu.stt_backend}")
            if self.gpu.stt_timestamps == "segment":
                raise ConfigError("HUB_STT_BEAM_SIZE > 1 does not combine with "
                                  "HUB_STT_TIMESTAMPS=segment (beams carry no timestamp rule state)")
            if self.gpu.stt_word_timestamps == "on":
                raise ConfigError("HUB_STT_BEAM_SIZE > 1 does not combine with "
                                  "HUB_STT_WORD_TIMESTAMPS=on (beams carry no query store)")
            if len(t) > 1:
                raise ConfigError("HUB_STT_BEAM_SIZE > 1 does not combine with a HUB_STT_TEMPERATURE "
                                  f"fallback list: {t}")
            if b > self.gpu.max_batch:
                raise ConfigError(f"HUB_STT_BEAM_SIZE {b} exceeds HUB_MAX_BATCH "
                                  f"{self.gpu.max_batch} (decoder rows)")
        if self.gpu.stt_hotwords_skills not in ("off", "on"):
            raise ConfigError("invalid HUB_STT_HOTWORDS_SKILLS (off | on): "
                              f"{self.gpu.stt_hotwords_skills}")
        hb = self.gpu.stt_hotword_boost
        if not (math.isfinite(hb) and abs(hb) <= 3.4028234663852886e38):
            raise ConfigError(f"HUB_STT_HOTWORD_BOOST must be a finite f32 number: {hb}")
        if len(self.gpu.stt_hotwords) > HOTWORD_MAX_PHRASES:
            raise ConfigError(f"HUB_STT_HOTWORDS: {len(self.gpu.stt_hotwords)} phrases exceed the "
                              f"limit of {HOTWORD_MAX_PHRASES}: "
                              f"{self.gpu.stt_hotwords[HOTWORD_MAX_PHRASES]!r}")
        if self.gpu.hotwords_on:
            if self.gpu.stt_backend != "gpu":
                raise ConfigError("HUB_STT_HOTWORDS / HUB_STT_HOTWORDS_SKILLS need "
                                  f"HUB_STT_BACKEND=gpu: {self.gpu.stt_backend}")
            if b > 1:
                raise ConfigError("HUB_STT_BEAM_SIZE > 1 does not combine with HUB_STT_HOTWORDS "
                                  "(beams carry no hotword state)")
        if self.gpu.stt_vad not in ("off", "on"):
            raise ConfigError(f"invalid HUB_STT_VAD (off | on): {self.gpu.stt_vad}")
        if self.gpu.stt_vad == "on" and self.gpu.stt_backend != "gpu":
            raise ConfigError(f"HUB_STT_VAD=on needs HUB_STT_BACKEND=gpu: {self.gpu.stt_backend}")
        try:
            # the bounds live with the detector's parameters (ops.reference.vad_params)
            self.gpu.vad_config(always=True)
        except ValueError as e:
            key = next((k for name, k in _VAD_KEYS.items() if f" {name} " in str(e)), "HUB_VAD_*")
            raise ConfigError(f"invalid {key}: {e}") from None
        if not self.gpu.stt_compression_ratio_threshold > 0.0:
            raise ConfigError("HUB_STT_COMPRESSION_RATIO_THRESHOLD must be > 0: "
                              f"{self.gpu.stt_compression_ratio_threshold}")
        for c in self.gpu.stt_languages:
            if not re.fullmatch(r"[a-z]{2,3}", c):
                raise ConfigError(f"invalid HUB_STT_LANGUAGES entry: {c!r}")


def parse_relay_groups(s: str) -> dict:
    """"relay-1=kitchen,relay-2=kitchen" -> {relay id: group}."""
    out = {}
    for part in filter(None, (p.strip() for p in s.split(","))):
        k, sep, v = part.partition("=")
        if sep and k.strip() and v.strip():
            out[k.strip()] = v.strip()
    return out


class ConfigError(ValueError):
    pass


def _tts_sample_rate(e) -> int:
    """``HUB_TTS_SAMPLE_RATE``: an integer (not silently the default: a typo
    would leave the relays playing the reply at the wrong speed)."""
    v = env_str(e, "0", "HUB_TTS_SAMPLE_RATE").strip()
    try:
        return int(v)
    except ValueError:
        raise ConfigError(f"invalid configuration: invalid HUB_TTS_SAMPLE_RATE: {v}") from None


def _tts_flac_block(e) -> int:
    """``HUB_TTS_FLAC_BLOCK``: an integer, checked against FLAC_BLOCK_SIZES by
    ``Config.validate``."""
    v = env_str(e, "4096", "HUB_TTS_FLAC_BLOCK").strip()
    try:
        return int(v)
    except ValueError:
        raise ConfigError(f"invalid configuration: invalid HUB_TTS_FLAC_BLOCK: {v}") from None


def _stt_language(e) -> str:
    """``STT_LANGUAGE``: unset = "en"; "auto", or set and empty (the reference
    passes an empty language through, and a Whisper service then detects it) =
    "auto"."""
    v = e.get("STT_LANGUAGE")
    if v is None:
        return "en"
    v = str(v).strip()
    return "auto" if v == "" or v.lower() == "auto" else v


def _strict_float(e, default: float, key: str) -> float:
    v = env_str(e, "", key).strip()
    if v == "":
        return default
    try:
        return float(v)
    except ValueError:
        raise ConfigError(f"invalid configuration: invalid {key}: {v}") from None


def _float_list(e, default: list, key: str) -> list:
    """A comma list of numbers ("0,0.2,0.4"); empty / unset: ``default``."""
    v = env_str(e, "", key).strip()
    if v == "":
        return list(default)
    try:
        return [float(x) for x in v.split(",")]
    except ValueError:
        raise ConfigError(f"invalid configuration: invalid {key}: {v}") from None


def _beam_size(e) -> int:
    """HUB_STT_BEAM_SIZE: an integer (its range is checked in ``validate``);
    empty / unset: 1, greedy decoding."""
    v = env_str(e, "", "HUB_STT_BEAM_SIZE").strip()
    if v == "":
        return 1
    if not re.fullmatch(r"[+-]?\d+", v):
        raise ConfigError(f"invalid configuration: invalid HUB_STT_BEAM_SIZE: {v}")
    return int(v)


def _strict_int(e, default: int, key: str) -> int:
    v = env_str(e, "", key).strip()
    if v == "":
        return default
    if not re.fullmatch(r"[+-]?\d+", v):
        raise ConfigError(f"invalid configuration: invalid {key}: {v}")
    return int(v)


def _hotword_list(phrases) -> list:
    """Phrases stripped, their inner whitespace collapsed, empty ones dropped,
    duplicates collapsed (the first kept)."""
    out, seen = [], set()
    for p in phrases:
        p = " ".join(str(p).split())
        if p and p not in seen:
            seen.add(p)
            out.append(p)
    return out


def _hotwords(e) -> list:
    """HUB_STT_HOTWORDS (a comma list) merged with the lines of
    HUB_STT_HOTWORDS_FILE (one phrase per line; blank lines and lines that
    start with ``#`` are skipped)."""
    out = env_str(e, "", "HUB_STT_HOTWORDS").split(",")
    path = env_str(e, "", "HUB_STT_HOTWORDS_FILE").strip()
    if path:
        try:
            with open(path, encoding="utf-8") as f:
                lines = f.read().splitlines()
        except OSError as err:
            raise ConfigError("invalid configuration: cannot read HUB_STT_HOTWORDS_FILE "
                              f"{path}: {err.strerror or err}") from None
        out += [ln for ln in lines if ln.strip() and not ln.lstrip().startswith("#")]
    return _hotword_list(out)


def load(env=None) -> Config:
    """Build the configuration from ``env`` (default ``os.environ``) and
    validate it; raises ``ConfigError`` ("invalid configuration: ...")."""
    e = os.environ if env is None else env
    c = Config(
        server=ServerConfig(
            host=env_str(e, "0.0.0.0", "LOQA_HOST"),
            port=env_int(e, 8080, "LOQA_PORT", "LOQA_HUB_PORT"),
            grpc_port=env_int(e, 50051, "LOQA_GRPC_PORT"),
            db_path=env_str(e, "./data/loqa-hub.db", "LOQA_DB_PATH", "DB_PATH"),
            read_timeout=env_duration(e, 30.0, "LOQA_READ_TIMEOUT"),
            write_timeout=env_duration(e, 30.0, "LOQA_WRITE_TIMEOUT"),
        ),
        stt=STTConfig(
            url=env_str(e, "http://stt:8000", "STT_URL"),
            language=_stt_language(e),
            temperature=env_float(e, 0.0, "STT_TEMPERATURE"),
            max_tokens=env_int(e, 224, "STT_MAX_TOKENS"),
        ),
        tts=TTSConfig(
            url=env_str(e, "http://localhost:8880/v1", "TTS_URL"),
            voice=env_str(e, "af_bella", "TTS_VOICE"),
            speed=env_float(e, 1.0, "TTS_SPEED"),
            response_format=env_str(e, "wav", "TTS_FORMAT"),
            normalize=env_bool(e, True, "TTS_NORMALIZE"),
            max_concurrent=env_int(e, 10, "TTS_MAX_CONCURRENT"),
            timeout=env_duration(e, 10.0, "TTS_TIMEOUT"),
            fallback_enabled=env_bool(e, True, "TTS_FALLBACK_ENABLED"),
        ),
        streaming=StreamingConfig(
            enabled=env_bool(e, False, "STREAMING_ENABLED"),
            ollama_url=env_str(e, "http://ollama:11434", "OLLAMA_URL", "STREAMING_OLLAMA_URL"),
            model=env_str(e, "llama3.2:3b", "STREAMING_MODEL"),
            max_buffer_time=env_duration(e, 2.0, "STREAMING_MAX_BUFFER_TIME"),
            max_tokens_per_phrase=env_int(e, 50, "STREAMING_MAX_TOKENS_PER_PHRASE"),
            audio_concurrency=env_int(e, 3, "STREAMING_AUDIO_CONCURRENCY"),
            visual_feedback_delay=env_duration(e, 0.050, "STREAMING_VISUAL_DELAY",
                                               "STREAMING_VISUAL_FEEDBACK_DELAY"),
            interrupt_timeout=env_duration(e, 0.500, "STREAMING_INTERRUPT_TIMEOUT"),
            fallback_enabled=env_bool(e, True, "STREAMING_FALLBACK_ENABLED"),
            metrics_enabled=env_bool(e, True, "STREAMING_METRICS_ENABLED"),
        ),
        logging=LoggingConfig(
            level=env_str(e, "info", "LOG_LEVEL"),
            format=env_str(e, "json", "LOG_FORMAT"),
        ),
        nats=NATSConfig(
            url=env_str(e, "nats://localhost:4222", "NATS_URL"),
            subject=env_str(e, "loqa.commands", "NATS_SUBJECT"),
            max_reconnect=env_int(e, 10, "NATS_MAX_RECONNECT"),
            reconnect_wait=env_duration(e, 2.0, "NATS_RECONNECT_WAIT"),
        ),
        privacy=PrivacyConfig(
            data_retention=env_duration(e, 30 * 24 * 3600.0, "LOQA_DATA_RETENTION"),
            zero_persistence=env_bool(e, False, "LOQA_ZERO_PERSISTENCE"),
            auto_cleanup_enabled=env_bool(e, True, "LOQA_AUTO_CLEANUP"),
            cleanup_interval=env_duration(e, 24 * 3600.0, "LOQA_CLEANUP_INTERVAL"),
        ),
        ollama=OllamaConfig(
            url=env_str(e, "http://localhost:11434", "OLLAMA_URL"),
            model=env_str(e, "llama3.2:3b", "OLLAMA_MODEL"),
        ),
        gpu=GPUConfig(
            num_gpus=env_int(e, 0, "HUB_NUM_GPUS"),
            dp=env_int(e, 0, "HUB_DP"),
            tp=env_int(e, 1, "HUB_TP"),
            stt_model=env_str(e, "whisper-base", "HUB_STT_MODEL"),
            llm_model=env_str(e, "tinyllama", "HUB_LLM_MODEL"),
            tts_model=env_str(e, "vits-ljs", "HUB_TTS_MODEL"),
            dtype=env_str(e, "bf16", "HUB_DTYPE"),
            max_batch=env_int(e, 64, "HUB_MAX_BATCH"),
            kv_block=env_int(e, 16, "HUB_KV_BLOCK"),
            max_seq_len=env_int(e, 1024, "HUB_MAX_SEQ_LEN"),
            llm_backend=env_str(e, "gpu", "HUB_LLM_BACKEND"),
            llm_weights=env_str(e, "bf16", "HUB_LLM_WEIGHTS").lower(),
            stt_backend=env_str(e, "gpu", "HUB_STT_BACKEND"),
            stt_confidence=env_str(e, "heuristic", "HUB_STT_CONFIDENCE").lower(),
            stt_confirm_below=env_float(e, 0.6, "HUB_STT_CONFIRM_BELOW"),
            stt_languages=[c.strip().lower() for c in
                           env_str(e, "", "HUB_STT_LANGUAGES").split(",") if c.strip()],
            stt_no_speech=env_str(e, "off", "HUB_STT_NO_SPEECH").strip().lower(),
            stt_no_speech_threshold=_strict_float(e, 0.6, "HUB_STT_NO_SPEECH_THRESHOLD"),
            stt_logprob_threshold=_strict_float(e, -1.0, "HUB_STT_LOGPROB_THRESHOLD"),
            stt_timestamps=env_str(e, "off", "HUB_STT_TIMESTAMPS").strip().lower(),
            stt_max_initial_timestamp=_strict_float(e, 1.0, "HUB_STT_MAX_INITIAL_TIMESTAMP"),
            stt_temperature=_float_list(e, [0.0], "HUB_STT_TEMPERATURE"),
            stt_word_timestamps=env_str(e, "off", "HUB_STT_WORD_TIMESTAMPS").strip().lower(),
            stt_alignment_heads="".join(env_str(e, "", "HUB_STT_ALIGNMENT_HEADS").split()),
            stt_beam_size=_beam_size(e),
            stt_hotwords=_hotwords(e),
            stt_hotwords_file=env_str(e, "", "HUB_STT_HOTWORDS_FILE").strip(),
            stt_hotword_boost=_strict_float(e, 2.0, "HUB_STT_HOTWORD_BOOST"),
            stt_hotwords_skills=env_str(e, "off", "HUB_STT_HOTWORDS_SKILLS").strip().lower(),
            stt_compression_ratio_threshold=_strict_float(e, 2.4,
                                                          "HUB_STT_COMPRESSION_RATIO_THRESHOLD"),
            stt_vad=env_str(e, "off", "HUB_STT_VAD").strip().lower(),
            vad_threshold_db=_strict_float(e, 9.0, "HUB_VAD_THRESHOLD_DB"),
            vad_min_level_dbfs=_strict_float(e, -55.0, "HUB_VAD_MIN_LEVEL_DBFS"),
            vad_floor_max_dbfs=_strict_float(e, -30.0, "HUB_VAD_FLOOR_MAX_DBFS"),
            vad_floor_s=_strict_float(e, 3.0, "HUB_VAD_FLOOR_S"),
            vad_min_speech_ms=_strict_int(e, 100, "HUB_VAD_MIN_SPEECH_MS"),
            vad_min_silence_ms=_strict_int(e, 500, "HUB_VAD_MIN_SILENCE_MS"),
            vad_pad_ms=_strict_int(e, 200, "HUB_VAD_PAD_MS"),
            audio_input_rate=env_str(e, "fixed", "HUB_AUDIO_INPUT_RATE").lower(),
            tts_sample_rate=_tts_sample_rate(e),
            tts_backend=env_str(e, "gpu", "HUB_TTS_BACKEND"),
            use_graphs=env_bool(e, True, "HUB_USE_GRAPHS"),
            seed=env_int(e, 0, "HUB_SEED"),
            tp_fallback_model=env_str(e, "llama3-8b", "HUB_TP_FALLBACK_MODEL"),
            tp_fallback_checkpoint=env_str(e, "", "HUB_TP_FALLBACK_CHECKPOINT"),
            stt_checkpoint=env_str(e, "", "HUB_STT_CHECKPOINT"),
            llm_checkpoint=env_str(e, "", "HUB_LLM_CHECKPOINT"),
            tts_checkpoint=env_str(e, "", "HUB_TTS_CHECKPOINT"),
            tts_format_policy=env_str(e, "wav", "HUB_TTS_FORMAT_POLICY"),
            tts_flac_block=_tts_flac_block(e),
            stt_tokenizer=env_str(e, "", "HUB_STT_TOKENIZER"),
            llm_tokenizer=env_str(e, "", "HUB_LLM_TOKENIZER"),
        ),
        arbitration=ArbitrationConfig(
            window=env_duration(e, 0.300, "ARBITRATION_WINDOW_DURATION"),
            scope=env_str(e, "global", "ARBITRATION_SCOPE"),
            max_concurrent_relays=env_int(e, 0, "MAX_CONCURRENT_RELAYS"),
            end_of_speech_wait=env_duration(e, 5.0, "ARBITRATION_EOS_WAIT"),
            bridge_timeout=env_duration(e, 2.0, "BRIDGE_TIMEOUT"),
            confirmation_enabled=env_bool(e, False, "CONFIRMATION_ENABLED"),
            relay_groups=parse_relay_groups(env_str(e, "", "ARBITRATION_RELAY_GROUPS")),
            single_relay_bypass=env_bool(e, False, "ARBITRATION_SINGLE_RELAY_BYPASS"),
        ),
    )
    try:
        c.validate()
    except ConfigError as err:
        raise ConfigError(f"invalid configuration: {err}") from err
    return c

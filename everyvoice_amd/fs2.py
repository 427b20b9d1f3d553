"""FastSpeech2 feature prediction (text ids -> mel), inference forward path on libevmi_hip.

Host-side mirror of what the reference constructs as ``FastSpeech2(config, stats=..., lang2id=..., speaker2id=...)``
(``everyvoice/tests/model_stubs.py:44-58``; the module itself lives in the absent submodule
EveryVoiceTTS/FastSpeech2_lightning).  Configuration names follow the reference's schema
(``everyvoice/.schema/everyvoice-text-to-spec-0.5.json``: ConformerConfig {layers, heads, input_dim, feedforward_dim,
conv_kernel_size, dropout}, VariancePredictorConfig {n_layers, kernel_size, input_dim, n_bins, depthwise, level}); the
state-dict layout is the one of ``torchaudio.models.Conformer`` for encoder / decoder (the ConformerConfig field set is
exactly that constructor) plus ``text_input_layer``, ``position_embedding.inv_freq`` (the tensor
``everyvoice/tests/data/test.ckpt`` holds), ``{duration,pitch,energy}_predictor``, ``{pitch,energy}_embedding``,
``mel_linear`` and ``postnet``.

Everything runs channel-major ``x[c][b][t]`` in fp32: Linear / pointwise / postnet layers on the fp32 matrix-core
implicit GEMM (``evmi_conv1d_cbt_f32``), attention, LayerNorm, depthwise convolutions (eval-mode BatchNorm and weight norm
folded at load time), embeddings, bucketisation, the integer length regulator in ``csrc/fs2_ops.hip``.  No CPU fallback.
"""

from __future__ import annotations

from dataclasses import dataclass, field
from typing import NamedTuple

import torch

from . import _lib
from .train import ops
from .train.ops import _chk, _s


@dataclass
class ConformerConfig:
    layers: int = 4
    heads: int = 2
    input_dim: int = 256
    feedforward_dim: int = 1024
    conv_kernel_size: int = 9
    dropout: float = 0.2


@dataclass
class VariancePredictorConfig:
    loss: str = "mse"
    n_layers: int = 5
    kernel_size: int = 3
    dropout: float = 0.5
    input_dim: int = 256
    n_bins: int = 256
    depthwise: bool = True
    level: str = "phone"


@dataclass
class StatsInfo:
    """``everyvoice/tests/model_stubs.py:50-57``."""
    min: float = -3.0
    max: float = 3.0
    std: float = 1.0
    mean: float = 0.0
    norm_min: float = -3.0
    norm_max: float = 3.0


@dataclass
class Stats:
    pitch: StatsInfo = field(default_factory=StatsInfo)
    energy: StatsInfo = field(default_factory=StatsInfo)


@dataclass
class VariancePredictors:
    energy: VariancePredictorConfig = field(default_factory=VariancePredictorConfig)
    duration: VariancePredictorConfig = field(default_factory=VariancePredictorConfig)
    pitch: VariancePredictorConfig = field(default_factory=VariancePredictorConfig)


@dataclass
class FastSpeech2ModelConfig:
    encoder: ConformerConfig = field(default_factory=ConformerConfig)
    decoder: ConformerConfig = field(default_factory=ConformerConfig)
    variance_predictors: VariancePredictors = field(default_factory=VariancePredictors)
    learn_alignment: bool = True
    max_length: int = 1000
    mel_loss: str = "mse"
    use_postnet: bool = True
    multilingual: bool = False
    multispeaker: bool = False
    # everyvoice-text-to-spec-0.5.json:265-272 (TargetTrainingTextRepresentationLevel): "characters" / "phones" = symbol ids through
    # the embedding table; "phonological_features" = 43-dim multi-hot vectors (text/features.py:7) through a bias-free Linear
    target_text_representation_level: str = "characters"
    # not in the reference's schema (fixed inside the absent module): sizes of the embedding table and the postnet
    n_symbols: int = 80
    n_mels: int = 80
    postnet_channels: int = 512
    postnet_kernel: int = 5
    postnet_layers: int = 5
    n_speakers: int = 0   # table sizes when multispeaker / multilingual (len(speaker2id) / len(lang2id) in the reference)
    n_languages: int = 0
    # everyvoice-text-to-spec-0.5.json:279-284: the Global Style Token module (arXiv 1803.09017) -- see StyleTokens below
    use_global_style_token_module: bool = False
    # not in the reference's schema (fixed inside the absent module; the GST paper's / GST-Tacotron's values)
    gst_num_heads: int = 8
    # the reference encoder treats frames beyond a reference's length as absent: the style embedding of an
    # utterance then does not depend on the padding or on what else is in its batch.  False = consume the padded tensor as torch.nn would
    gst_mask_padding: bool = False
    gst_num_tokens: int = 10
    gst_ref_enc_filters: tuple = (32, 32, 64, 64, 128, 128)
    # not in the reference's schema: every layer that looks beyond its own column (the Conformers' depthwise convolutions and, in
    # training, their BatchNorms; the variance predictors' k > 1 convolutions; the postnet) treats the columns at or beyond an item's
    # length as absent: what the model writes for an utterance then does not depend on the padding or on what
    # else is in its batch.  False = the padded columns are computed and seen, as in the reference's Conformer
    mask_padding: bool = False

    def __post_init__(self):
        self.gst_ref_enc_filters = tuple(int(v) for v in self.gst_ref_enc_filters)  # (a list after a JSON round trip)


N_PHONOLOGICAL_FEATURES = 43  # everyvoice/text/features.py:7

_LN_EPS = 1e-5
_BN_EPS = 1e-5


def _conv(x, w, b, k=1, act=ops.ACT_NONE):
    return ops.conv1d_mfma(x, w, b, 1, (k - 1) // 2, 1, 1, act=act)


def _conv_add(x, w, b, res, k=1):
    """res + conv(x): the residual is added in the convolution's epilogue on the packed bf16 kernels (one pass over the output
    instead of three); elsewhere the convolution and the sum run as before."""
    return ops.conv1d_fused_fwd(x, w, b, 1, (k - 1) // 2, 1, 1, residual=res)


def _layernorm(x, g, b):
    y = torch.empty_like(x)
    _chk(_lib.load().evmi_layernorm_cbt_f32(x.data_ptr(), g.data_ptr(), b.data_ptr(), y.data_ptr(), x.shape[0], x.shape[1] * x.shape[2],
                                            _LN_EPS, _s(x)), "evmi_layernorm_cbt_f32")
    return y


def _ln_conv(x, g, b, w, bias, act=ops.ACT_NONE):
    """act(conv1x1(LayerNorm(x))): on the packed bf16 kernels the normalised tensor is written straight into the convolution's packed input
    (ops.layernorm_dense_fwd: one launch and one fp32 round trip of the tensor less); elsewhere the two operators."""
    C, B, T = x.shape
    # (a position-wise layer: all columns as ONE item -- any B * T then shares the packed layout, csrc/conv_pk_common.h)
    if ops.ln_dense_fused_supported(1, B * T, C, w.shape[0]):
        return ops.layernorm_dense_fwd(x.reshape(C, 1, B * T), g, b, w, bias, {}, act=act, eps=_LN_EPS).view(-1, B, T)
    if ops.ln_dense_fused_supported(B, T, C, w.shape[0]):
        return ops.layernorm_dense_fwd(x, g, b, w, bias, {}, act=act, eps=_LN_EPS)
    return _conv(_layernorm(x, g, b), w, bias, act=act)


def _mask_cols_(x, lens):
    """x [C, B, T]: zero at the columns t >= lens[b], in place."""
    C, B, T = x.shape
    _chk(_lib.load().evmi_mask_cols_f32(x.data_ptr(), lens.data_ptr(), C, B, T, _s(x)), "evmi_mask_cols_f32")
    return x


def _dwconv(x, w, b, k, act, lens=None):
    """``lens`` (int32 [B] on the device; ``mask_padding``): the columns at or beyond lens[b] are absent -- read as zero, written as zero."""
    y = torch.empty_like(x)
    C, B, T = x.shape
    if lens is not None:
        _chk(_lib.load().evmi_dwconv1d_cbt_lens_f32(x.data_ptr(), w.data_ptr(), b.data_ptr(), lens.data_ptr(), y.data_ptr(), C, B, T, k, (k - 1) // 2,
                                                    act, _s(x)), "evmi_dwconv1d_cbt_lens_f32")
        return y
    _chk(_lib.load().evmi_dwconv1d_cbt_f32(x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), C, B, T, k, (k - 1) // 2, act, _s(x)),
         "evmi_dwconv1d_cbt_f32")
    return y


def _fold_weight_norm(sd, prefix):
    g, v = sd[prefix + ".weight_g"].float(), sd[prefix + ".weight_v"].float()
    return g * v / v.flatten(1).norm(dim=1).view(-1, *([1] * (v.dim() - 1)))


def _fold_bn(w, b, sd, prefix):
    """Eval-mode BatchNorm1d after a convolution: y = (conv - mean) / sqrt(var + eps) * gamma + beta."""
    s = sd[prefix + ".weight"].float() / torch.sqrt(sd[prefix + ".running_var"].float() + _BN_EPS)
    return w * s.view(-1, *([1] * (w.dim() - 1))), (b - sd[prefix + ".running_mean"].float()) * s + sd[prefix + ".bias"].float()


def variance_settings(c: "FastSpeech2ModelConfig") -> dict:
    """The three settings of the schema that choose an axis or a loss, validated and as plain strings:
    ``{"level": {"duration", "pitch", "energy"}, "loss": {"duration", "pitch", "energy", "mel"}}``.  ``level``: "phone" (the predictor and its
    bucket embedding on the symbol axis, in front of the length regulator) or "frame" (on the frame axis, behind it; durations exist on the
    symbol axis only, so ``duration.level`` is checked against the schema and has no effect); ``loss``: "mse" or "mae" (``mel`` = ``mel_loss``, for
    the mel and the postnet terms).  Enum objects are taken by their ``.value``; anything else raises ``ValueError``.  The configuration
    itself is not touched: ``apply_variance_settings`` is what a constructor calls."""
    vp = c.variance_predictors
    out = {"level": {}, "loss": {}}
    for name in ("duration", "pitch", "energy"):
        cfg = getattr(vp, name)
        level, loss = getattr(cfg.level, "value", cfg.level), getattr(cfg.loss, "value", cfg.loss)
        if level not in ("phone", "frame"):
            raise ValueError(f"model.variance_predictors.{name}.level: 'phone' or 'frame', got {level!r}")
        if loss not in ("mse", "mae"):
            raise ValueError(f"model.variance_predictors.{name}.loss: 'mse' or 'mae', got {loss!r}")
        out["level"][name], out["loss"][name] = level, loss
    mel_loss = getattr(c.mel_loss, "value", c.mel_loss)
    if mel_loss not in ("mse", "mae"):
        raise ValueError(f"model.mel_loss: 'mse' or 'mae', got {mel_loss!r}")
    out["loss"]["mel"] = mel_loss
    return out


def apply_variance_settings(c: "FastSpeech2ModelConfig") -> dict:
    """``variance_settings(c)``, refusing a value outside the schema where the configuration is read (not inside the first step), with
    the plain strings written back into ``c``: the hyper-parameters of a checkpoint are JSON only, and a configuration may arrive
    holding enum objects.  What the model, the trainer and ``lightning.FastSpeech2Config`` call when they take a configuration over."""
    out = variance_settings(c)
    for name in ("duration", "pitch", "energy"):
        cfg = getattr(c.variance_predictors, name)
        cfg.level, cfg.loss = out["level"][name], out["loss"][name]
    c.mel_loss = out["loss"]["mel"]
    return out


def check_conformer_widths(c: "FastSpeech2ModelConfig") -> None:
    """Refuses, where the configuration is read (not inside the first forward or training step), an encoder / decoder whose width the
    kernels do not run: ``input_dim`` must be even (the sinusoidal positional term has ``input_dim / 2`` frequencies) and a multiple of
    ``heads``, and the head dimension ``input_dim / heads`` at most 256 (csrc/attention_generic.hip; 32 / 64 / 128 run on the specialised
    kernels), and ``input_dim`` itself at most 1024, the widest column the LayerNorm kernels (forward, backward, packed) normalise.
    ``ValueError`` naming the field.  Called by the model, the trainer and ``lightning.FastSpeech2Config``."""
    for name in ("encoder", "decoder"):
        cf = getattr(c, name)
        d, heads = int(cf.input_dim), int(cf.heads)
        if d <= 0 or d % 2:
            raise ValueError(f"model.{name}.input_dim: must be positive and even, got {d}")
        if heads <= 0 or d % heads:
            raise ValueError(f"model.{name}.heads: input_dim {d} is not a multiple of heads {heads}")
        if d // heads > ops.ATTENTION_MAX_HEAD_DIM:
            raise ValueError(f"model.{name}.heads: the head dimension input_dim / heads = {d} / {heads} = {d // heads} is above "
                             f"{ops.ATTENTION_MAX_HEAD_DIM}, the largest the attention kernels take")
        if d > ops.LAYERNORM_MAX_CHANNELS:
            raise ValueError(f"model.{name}.input_dim: {d} is above {ops.LAYERNORM_MAX_CHANNELS}, the widest the LayerNorm kernels take")


def gst_state_dict_shapes(c: "FastSpeech2ModelConfig") -> dict:
    """THE key-name table of the Global Style Token module: every tensor of its state dict except ``num_batches_tracked`` (which the
    trainer adds for each ``bns.{i}``), in declaration order.  The module lives in the absent FastSpeech2_lightning submodule, so the
    names and the layout follow the public lineage (KinglittleQ/GST-Tacotron, mozilla/TTS); to load a real checkpoint, map its keys
    HERE -- the inference model and the trainer both take their names from this function.
    With E = encoder.input_dim: reference encoder = len(filters) x [Conv2d(k 3, stride 2, padding 1) -> BatchNorm2d -> ReLU] over the mel
    as a one-channel image [B, 1, T, n_mels], then GRU(filters[-1] * n_mels' -> E / 2), last hidden state; style token layer = `tokens`
    embeddings of E / heads, keys and values from tanh(embed), bias-free W_query (E / 2 -> E), W_key, W_value (E / heads -> E)."""
    E, heads = c.encoder.input_dim, c.gst_num_heads
    if E % 2 or E % heads:
        raise ValueError(f"Global Style Token module: encoder.input_dim {E} must be even and a multiple of gst_num_heads {heads}")
    # what csrc/gst.hip is built for: the GRU keeps W_hh in registers at a hidden size of 32, 64 or 128; at most 16 tokens
    if E not in (64, 128, 256):
        raise ValueError(f"Global Style Token module: encoder.input_dim {E} is not supported (the GRU kernels exist for a hidden size "
                         "E / 2 of 32, 64 or 128, i.e. encoder.input_dim 64, 128 or 256)")
    if not 1 <= c.gst_num_tokens <= 16:
        raise ValueError(f"Global Style Token module: gst_num_tokens {c.gst_num_tokens} is not supported (1 to 16 tokens)")
    if not c.gst_ref_enc_filters:
        raise ValueError("Global Style Token module: gst_ref_enc_filters is empty")
    shapes, cin, bins = {}, 1, c.n_mels
    for i, cout in enumerate(c.gst_ref_enc_filters):
        shapes[f"gst.encoder.convs.{i}.weight"], shapes[f"gst.encoder.convs.{i}.bias"] = (cout, cin, 3, 3), (cout,)
        for leaf in ("weight", "bias", "running_mean", "running_var"):
            shapes[f"gst.encoder.bns.{i}.{leaf}"] = (cout,)
        cin, bins = cout, (bins - 1) // 2 + 1
    H = E // 2
    shapes.update({"gst.encoder.gru.weight_ih_l0": (3 * H, cin * bins), "gst.encoder.gru.weight_hh_l0": (3 * H, H),
                   "gst.encoder.gru.bias_ih_l0": (3 * H,), "gst.encoder.gru.bias_hh_l0": (3 * H,),
                   "gst.stl.embed": (c.gst_num_tokens, E // heads), "gst.stl.attention.W_query.weight": (E, H),
                   "gst.stl.attention.W_key.weight": (E, E // heads), "gst.stl.attention.W_value.weight": (E, E // heads)})
    return shapes


ALIGNER_CHANNELS = 80  # the attention dimension of the aligner (``train.fs2._AlignerT.n_att``)


def aligner_state_dict_shapes(c: "FastSpeech2ModelConfig") -> dict:
    """Names and shapes of the aligner of ``learn_alignment: true`` as the trainer declares them (``train.fs2._AlignerT``; FastPitch
    ``ConvAttention``): keys = Conv(k 3) - ReLU - Conv(1) over the symbol embeddings, queries = Conv(k 3) - ReLU - Conv(1) - ReLU -
    Conv(1) over the mel.  A checkpoint of a model trained with a learnt alignment holds them; ``FastSpeech2.load_state_dict`` takes
    them when all are there, and ``FastSpeech2.align`` then finds an utterance's durations from its own mel."""
    d, m, n = c.encoder.input_dim, c.n_mels, ALIGNER_CHANNELS
    shapes = {}
    for name, (cout, cin, k) in (("key_proj.0", (2 * d, d, 3)), ("key_proj.2", (n, 2 * d, 1)),
                                 ("query_proj.0", (2 * m, m, 3)), ("query_proj.2", (m, 2 * m, 1)), ("query_proj.4", (n, m, 1))):
        shapes[f"attention.{name}.conv.weight"], shapes[f"attention.{name}.conv.bias"] = (cout, cin, k), (cout,)
    return shapes


class StyleTokens:
    """Global Style Token module, inference: a reference mel [B, T, n_mels] -> a style embedding [B, E] that is added to the encoder
    output at every non-padded text position (where the speaker / language embeddings go).  Eval-mode BatchNorm is folded into the
    convolutions at load time and the keys / values of the (constant) tokens are computed once; everything runs in fp32 in both
    precision modes.  The mel is consumed as given, zero padding included (no length masking: ``torch.nn`` semantics)."""

    def __init__(self, c: "FastSpeech2ModelConfig", sd: dict, dev):
        put = lambda t: t.to(dev, torch.float32).contiguous()
        self.heads, self.n_mels = c.gst_num_heads, c.n_mels
        self.convs = []
        for i in range(len(c.gst_ref_enc_filters)):
            w, b = _fold_bn(sd[f"gst.encoder.convs.{i}.weight"].float(), sd[f"gst.encoder.convs.{i}.bias"].float(), sd, f"gst.encoder.bns.{i}")
            self.convs.append((put(w), put(b)))
        g = "gst.encoder.gru."
        self.w_ih, self.b_ih = put(sd[g + "weight_ih_l0"].unsqueeze(-1)), put(sd[g + "bias_ih_l0"])
        self.w_hh, self.b_hh = put(sd[g + "weight_hh_l0"]), put(sd[g + "bias_hh_l0"])
        a = "gst.stl.attention."
        tokens = torch.tanh(sd["gst.stl.embed"].float().cpu())
        self.keys = put(sd[a + "W_key.weight"].float().cpu() @ tokens.t())      # [E, tokens]
        self.values = put(sd[a + "W_value.weight"].float().cpu() @ tokens.t())
        self.w_q = put(sd[a + "W_query.weight"].unsqueeze(-1))

    def forward(self, mel: torch.Tensor, lens: torch.Tensor | None = None) -> torch.Tensor:
        """``lens`` (int32 [B] on the device, 1 <= lens[b] <= T): frames at or beyond lens[b] are absent, whatever they hold -- row b is
        the embedding of that reference alone at its own length.  None: the mel is consumed as given."""
        B, T, F = mel.shape
        x = mel.view(1, B, T, F)
        rows = [lens] + ops.gst_valid_rows(lens, len(self.convs)) if lens is not None else [None] * (len(self.convs) + 1)
        for (w, b), n in zip(self.convs, rows):
            x = ops.gst_conv2d_fwd(x, w, b, ops.ACT_RELU, rows=n)
        C, _, T2, F2 = x.shape
        seq = x.permute(0, 3, 1, 2).reshape(C * F2, 1, B * T2)  # the GRU's input features: channel-major (c, bin), one column per (item, step)
        with ops.exact_f32():
            gi = ops.conv1d_fwd(seq, self.w_ih, self.b_ih).view(-1, B, T2)
            h, _ = ops.gst_gru_fwd(gi, self.w_hh, self.b_hh, save=False, steps=rows[-1])
            q = ops.conv1d_fwd(h.view(-1, 1, B), self.w_q, None).view(-1, B)
        return ops.gst_attention_fwd(q, self.keys, self.values, self.heads, save=False)[0]


def check_style_lens(style_lens, style_mel_shape, what="style_lens"):
    """Host-side refusals for the per-reference lengths that go with ``style_mel`` [n, Ts, n_mels]: ``style_lens`` must be an integer
    [n] with 1 <= length <= Ts.  Values are looked at only where the lengths live on the host (a device tensor is not synchronised
    with); the kernels clamp what they read."""
    if style_lens is None:
        return None
    if style_mel_shape is None:
        raise ValueError(f"`{what}` given without `style_mel`")
    if not isinstance(style_lens, torch.Tensor):
        style_lens = torch.as_tensor(style_lens)
    n, Ts = int(style_mel_shape[0]), int(style_mel_shape[1])
    if style_lens.dim() != 1 or style_lens.shape[0] != n or style_lens.dtype.is_floating_point or style_lens.dtype == torch.bool:
        raise ValueError(f"{what}: expected {n} integer lengths (one per row of style_mel), got {style_lens.dtype} {tuple(style_lens.shape)}")
    if style_lens.device.type == "cpu" and n and (int(style_lens.min()) < 1 or int(style_lens.max()) > Ts):
        raise ValueError(f"{what}: lengths must be between 1 and Ts = {Ts}, got {style_lens.tolist()}")
    return style_lens


FIT_MAX_SYMBOLS = _lib.EVMI_FS2_FIT_MAX_SYMBOLS  # the longest text ``target_frames`` takes (evmi_fs2_fit_durations_i32)


def _is_scalar_control(control) -> bool:
    """One number for the whole batch: whatever ``float()`` takes (a Python or numpy number, a tensor of one element and no axis)."""
    if isinstance(control, torch.Tensor) and control.dim() > 0:
        return False
    try:
        float(control)
    except (TypeError, ValueError):
        return False
    return True


def check_prosody_arguments(B: int, L: int, levels: dict | None = None, duration_control=1.0, pitch_control=1.0, energy_control=1.0,
                            pitch=None, energy=None, target_frames=None, durations=None) -> None:
    """Host-side refusals for the steering arguments of ``FastSpeech2.__call__``, for a batch of ``B`` items of
    ``L`` symbols; ``levels``: ``{"pitch": "phone" | "frame", "energy": ...}`` (default: both "phone").  ``ValueError``, before any launch:
    a control that is neither a number nor a floating-point tensor [B, L] or [B]; a forced ``pitch`` / ``energy`` that is not a
    floating-point [B, L] (phone level) or [B, T'] (frame level), or that comes with a non-default control of the same variance (a
    forced value is embedded as given: the control would be ignored); ``target_frames`` that is not an integer [B], that comes with
    ``durations``, or with a text above ``FIT_MAX_SYMBOLS`` symbols; a negative target.  Values are looked at only where the tensor lives
    on the host (a device tensor is not synchronised with; the fit kernel takes a target below 1 as no target)."""
    levels = levels or {}
    controls = {"duration": duration_control, "pitch": pitch_control, "energy": energy_control}
    for name, control in controls.items():
        if _is_scalar_control(control):
            continue
        if not isinstance(control, torch.Tensor) or not control.dtype.is_floating_point or tuple(control.shape) not in ((B, L), (B,)):
            what = f"{control.dtype} {tuple(control.shape)}" if isinstance(control, torch.Tensor) else type(control).__name__
            raise ValueError(f"{name}_control: a number, or a floating-point tensor [{B}, {L}] (per symbol) or [{B}] (per item), got {what}")
    for name, forced in (("pitch", pitch), ("energy", energy)):
        if forced is None:
            continue
        level = levels.get(name, "phone")
        ok = isinstance(forced, torch.Tensor) and forced.dtype.is_floating_point and forced.dim() == 2 and forced.shape[0] == B \
            and (forced.shape[1] == L if level == "phone" else forced.shape[1] >= 1)
        if not ok:
            what = f"{forced.dtype} {tuple(forced.shape)}" if isinstance(forced, torch.Tensor) else type(forced).__name__
            raise ValueError(f"{name}: forced values of a {level}-level predictor are a floating-point tensor "
                             + (f"[{B}, {L}]" if level == "phone" else f"[{B}, T'] with T' at least the longest item's frames") + f", got {what}")
        if not (_is_scalar_control(controls[name]) and float(controls[name]) == 1.0):
            raise ValueError(f"{name} is forced and {name}_control is given: forced values are embedded as they are, a control would be ignored")
    if target_frames is not None:
        if durations is not None:
            raise ValueError("target_frames and durations are both given: given durations already fix every item's length")
        t = target_frames
        if not isinstance(t, torch.Tensor) or t.dtype.is_floating_point or t.dtype == torch.bool or tuple(t.shape) != (B,):
            what = f"{t.dtype} {tuple(t.shape)}" if isinstance(t, torch.Tensor) else type(t).__name__
            raise ValueError(f"target_frames: an integer tensor [{B}] (0 = no target for that item), got {what}")
        if t.device.type == "cpu" and B and int(t.min()) < 0:
            raise ValueError(f"target_frames: a target cannot be negative, got {t.tolist()}")
        if L > FIT_MAX_SYMBOLS:
            raise ValueError(f"target_frames: a text of {L} symbols is above the {FIT_MAX_SYMBOLS} the fit takes")


class _Conformer:
    def __init__(self, cfg: ConformerConfig, sd: dict, prefix: str, dev, mask_padding: bool = False):
        self.cfg, self.mask_padding = cfg, mask_padding
        self.layers = []
        d = cfg.input_dim
        put = lambda t: t.to(dev, torch.float32).contiguous()
        for i in range(cfg.layers):
            p = f"{prefix}.conformer_layers.{i}."
            L = {}
            for name in ("ffn1", "ffn2"):
                L[name] = dict(ln_g=put(sd[p + name + ".sequential.0.weight"]), ln_b=put(sd[p + name + ".sequential.0.bias"]),
                               w1=put(sd[p + name + ".sequential.1.weight"].unsqueeze(-1)), b1=put(sd[p + name + ".sequential.1.bias"]),
                               # the block's 0.5 (x + 0.5 * ffn(x)) is folded into the second layer: scaling by a power of two is
                               # exact, so res + conv(h, w2 / 2, b2 / 2) rounds exactly as x + 0.5 * conv(h, w2, b2) did
                               w2=put(0.5 * sd[p + name + ".sequential.4.weight"].float().unsqueeze(-1)),
                               b2=put(0.5 * sd[p + name + ".sequential.4.bias"].float()))
            L["attn"] = dict(ln_g=put(sd[p + "self_attn_layer_norm.weight"]), ln_b=put(sd[p + "self_attn_layer_norm.bias"]),
                             w_in=put(sd[p + "self_attn.in_proj_weight"].unsqueeze(-1)), b_in=put(sd[p + "self_attn.in_proj_bias"]),
                             w_out=put(sd[p + "self_attn.out_proj.weight"].unsqueeze(-1)), b_out=put(sd[p + "self_attn.out_proj.bias"]))
            c = p + "conv_module."
            wdw, bdw = _fold_bn(sd[c + "sequential.2.weight"].float(), sd[c + "sequential.2.bias"].float(), sd, c + "sequential.3")
            L["conv"] = dict(ln_g=put(sd[c + "layer_norm.weight"]), ln_b=put(sd[c + "layer_norm.bias"]),
                             w_pw1=put(sd[c + "sequential.0.weight"]), b_pw1=put(sd[c + "sequential.0.bias"]),
                             w_dw=put(wdw.reshape(d, -1)), b_dw=put(bdw),
                             w_pw2=put(sd[c + "sequential.5.weight"]), b_pw2=put(sd[c + "sequential.5.bias"]))
            L["final"] = dict(g=put(sd[p + "final_layer_norm.weight"]), b=put(sd[p + "final_layer_norm.bias"]))
            self.layers.append(L)

    def _ffn(self, x, P):
        C, B, T = x.shape
        if ops.ffn_packed_supported(1, B * T, C, P["w1"].shape[0], P["w2"].shape[0]):
            # the block as a packed chain (train/ops.py: ffn_packed_infer): the 1024-channel tensor exists as packed bf16 only
            xr = x.reshape(C, 1, B * T)
            return ops.ffn_packed_infer(xr, P["ln_g"], P["ln_b"], P["w1"], P["b1"], P["w2"], P["b2"], xr, eps=_LN_EPS).view(C, B, T)
        h = _ln_conv(x, P["ln_g"], P["ln_b"], P["w1"], P["b1"], act=ops.ACT_SILU)
        return _conv_add(h, P["w2"], P["b2"], x)

    def forward(self, x, lens):
        """x [D, B, T] (padded positions are computed, not masked: the convolution module sees them, as in the reference).  With
        ``mask_padding`` the depthwise convolution takes the columns at or beyond lens[b] as absent; attention masks its keys by length
        already and everything else is position-wise, so a valid column then depends on its own item's valid columns only."""
        lib = _lib.load()
        D, B, T = x.shape
        for L in self.layers:
            x = self._ffn(x, L["ffn1"])
            A = L["attn"]
            qkv = _ln_conv(x, A["ln_g"], A["ln_b"], A["w_in"], A["b_in"])
            att = torch.empty_like(x)
            attn = getattr(lib, ops.attention_entry("infer", D // self.cfg.heads))
            _chk(attn(qkv.data_ptr(), lens.data_ptr(), att.data_ptr(), B, T, D, self.cfg.heads, _s(x)), "evmi_attention_cbt")
            x = _conv_add(att, A["w_out"], A["b_out"], x)
            Cm = L["conv"]
            p = _ln_conv(x, Cm["ln_g"], Cm["ln_b"], Cm["w_pw1"], Cm["b_pw1"])
            g = ops.elementwise(15, p[:D], p[D:])  # GLU over the channel halves
            h = _dwconv(g, Cm["w_dw"], Cm["b_dw"], self.cfg.conv_kernel_size, 1, lens if self.mask_padding else None)  # depthwise + folded BatchNorm + SiLU
            x = _conv_add(h, Cm["w_pw2"], Cm["b_pw2"], x)
            x = self._ffn(x, L["ffn2"])
            x = _layernorm(x, L["final"]["g"], L["final"]["b"])
        return x


class _VariancePredictor:
    def __init__(self, cfg: VariancePredictorConfig, sd: dict, prefix: str, dev, mask_padding: bool = False):
        self.cfg, self.mask_padding = cfg, mask_padding
        put = lambda t: t.to(dev, torch.float32).contiguous()
        self.layers = []
        d = cfg.input_dim
        for i in range(cfg.n_layers):
            p = f"{prefix}.convs.{i}"
            if cfg.depthwise:
                conv = dict(w_dw=put(_fold_weight_norm(sd, p + ".0").reshape(d, -1)), b_dw=put(sd[p + ".0.bias"]),
                            w_pw=put(_fold_weight_norm(sd, p + ".1")), b_pw=put(sd[p + ".1.bias"]))
            else:
                conv = dict(w=put(sd[p + ".weight"]), b=put(sd[p + ".bias"]))
            conv.update(ln_g=put(sd[f"{prefix}.norms.{i}.weight"]), ln_b=put(sd[f"{prefix}.norms.{i}.bias"]))
            self.layers.append(conv)
        self.w_lin, self.b_lin = put(sd[prefix + ".linear.weight"].unsqueeze(-1)), put(sd[prefix + ".linear.bias"])

    def forward(self, x, lens):
        """x [D, B, L] -> [B, L] (zero at padded positions).  With ``mask_padding`` every layer's k > 1 convolution reads the columns at
        or beyond lens[b] as zero (layer 0 too: the caller's tensor holds bucket embeddings there); x itself is left as it is."""
        k = self.cfg.kernel_size
        mlens = lens if self.mask_padding else None
        for P in self.layers:
            if self.cfg.depthwise:
                h = _conv(_dwconv(x, P["w_dw"], P["b_dw"], k, 0, mlens), P["w_pw"], P["b_pw"], act=ops.ACT_RELU)
            else:
                if mlens is not None and k > 1:  # (a copy at layer 0: the tensor is the caller's; the LayerNorm outputs are this function's)
                    x = _mask_cols_(x.clone() if P is self.layers[0] else x, mlens)
                h = _conv(x, P["w"], P["b"], k, act=ops.ACT_RELU)
            x = _layernorm(h, P["ln_g"], P["ln_b"])
        y = _conv(x, self.w_lin, self.b_lin)  # [1, B, L]
        return _mask_cols_(y, lens)[0]


class AlignmentScores(NamedTuple):
    """What ``FastSpeech2.align(return_scores=True)`` says about an alignment (float32 on the device)."""

    ctc: torch.Tensor     # [B]    CTC forward-sum loss of the utterance aligned alone, divided by its symbols (the trainer's loss, without a batch's padding)
    path: torch.Tensor    # [B]    binarisation loss on the path of the durations: -mean over the frames of log soft attention
    symbol: torch.Tensor  # [B, L] mean log soft attention of each symbol over its own frames; 0 at padded symbols


class FastSpeech2:
    """``model = FastSpeech2(config, stats); model.load_state_dict(sd); mel, post, durations, pitch, energy, mel_lens = model(ids, lens)``

    ``variance_predictors.{pitch,energy}.level`` places each predictor and its bucket embedding: "phone" = on the symbol axis in front
    of the length regulator, "frame" = on the frame axis behind it (pitch, then energy, on either axis; the positional term of the
    decoder comes after both).  A frame-level predictor returns its values as [B, T]."""

    def __init__(self, config: FastSpeech2ModelConfig | None = None, stats: Stats | None = None, device="cuda:0",
                 lang2id: dict | None = None, speaker2id: dict | None = None, precision: str = "f32"):
        if precision not in ("f32", "bf16"):
            raise ValueError("precision: 'f32' (exact fp32 arithmetic) or 'bf16' (bf16 operands of the dense layers, fp32 accumulation)")
        self.precision = precision
        self.config = config or FastSpeech2ModelConfig()
        self.stats = stats or Stats()
        self.device = torch.device(device)
        self.lang2id, self.speaker2id = lang2id or {}, speaker2id or {}
        self.audio_config = None  # the model's preprocessing.audio, where the caller knows it: the synthesis helpers make a style reference's mel with it
        self.levels = apply_variance_settings(self.config)["level"]
        check_conformer_widths(self.config)
        if self.config.use_global_style_token_module:
            gst_state_dict_shapes(self.config)  # (refuses a size the kernels are not built for here, not inside the first forward)
        if self.device.type != "cuda":
            raise RuntimeError("FastSpeech2 runs on libevmi_hip (MI355X) only; there is no CPU path")
        _lib.load()
        self._ready = False

    # -- parameters -----------------------------------------------------------------------------------------------
    def load_state_dict(self, sd: dict):
        c, dev = self.config, self.device
        put = lambda t: t.to(dev, torch.float32).contiguous()
        self.table = put(sd["text_input_layer.weight"])
        self.inv_freq = put(sd["position_embedding.inv_freq"])
        self.encoder = _Conformer(c.encoder, sd, "encoder", dev, c.mask_padding)
        self.decoder = _Conformer(c.decoder, sd, "decoder", dev, c.mask_padding)
        self.speaker_table = put(sd["speaker_embedding.weight"]) if c.multispeaker else None
        self.language_table = put(sd["language_embedding.weight"]) if c.multilingual else None
        self.gst = StyleTokens(c, sd, dev) if c.use_global_style_token_module else None
        vp = c.variance_predictors
        self.duration_predictor = _VariancePredictor(vp.duration, sd, "duration_predictor", dev, c.mask_padding)
        self.pitch_predictor = _VariancePredictor(vp.pitch, sd, "pitch_predictor", dev, c.mask_padding)
        self.energy_predictor = _VariancePredictor(vp.energy, sd, "energy_predictor", dev, c.mask_padding)
        lin = lambda st, n: torch.linspace(st.norm_min, st.norm_max, n - 1)
        self.pitch_bins = put(sd["pitch_bins"] if "pitch_bins" in sd else lin(self.stats.pitch, vp.pitch.n_bins))
        self.energy_bins = put(sd["energy_bins"] if "energy_bins" in sd else lin(self.stats.energy, vp.energy.n_bins))
        self.pitch_table, self.energy_table = put(sd["pitch_embedding.weight"]), put(sd["energy_embedding.weight"])
        self.w_mel, self.b_mel = put(sd["mel_linear.weight"].unsqueeze(-1)), put(sd["mel_linear.bias"])
        self.postnet = []
        if c.use_postnet:
            for i in range(c.postnet_layers):
                p = f"postnet.convolutions.{i}"
                w, b = _fold_bn(sd[p + ".0.weight"].float(), sd[p + ".0.bias"].float(), sd, p + ".1")
                self.postnet.append((put(w), put(b)))
        names = aligner_state_dict_shapes(c)
        self.aligner = {n: put(sd[n]) for n in names} if c.learn_alignment and all(n in sd for n in names) else None
        self._ready = True
        return self

    @property
    def has_aligner(self) -> bool:
        """The loaded state dict held every tensor of ``aligner_state_dict_shapes`` (and ``learn_alignment`` is on): ``align`` works."""
        return getattr(self, "aligner", None) is not None

    @staticmethod
    def state_dict_shapes(c: FastSpeech2ModelConfig) -> dict:
        """Names and shapes of the state dict (``torchaudio.models.Conformer`` layout for encoder / decoder)."""
        pfs = c.target_text_representation_level == "phonological_features"
        shapes = {"text_input_layer.weight": (c.encoder.input_dim, N_PHONOLOGICAL_FEATURES) if pfs else (c.n_symbols, c.encoder.input_dim),
                  "position_embedding.inv_freq": (c.encoder.input_dim // 2,)}
        for name, cf in (("encoder", c.encoder), ("decoder", c.decoder)):
            d, f, k = cf.input_dim, cf.feedforward_dim, cf.conv_kernel_size
            for i in range(cf.layers):
                p = f"{name}.conformer_layers.{i}."
                for ffn in ("ffn1", "ffn2"):
                    shapes.update({p + ffn + ".sequential.0.weight": (d,), p + ffn + ".sequential.0.bias": (d,),
                                   p + ffn + ".sequential.1.weight": (f, d), p + ffn + ".sequential.1.bias": (f,),
                                   p + ffn + ".sequential.4.weight": (d, f), p + ffn + ".sequential.4.bias": (d,)})
                shapes.update({p + "self_attn_layer_norm.weight": (d,), p + "self_attn_layer_norm.bias": (d,),
                               p + "self_attn.in_proj_weight": (3 * d, d), p + "self_attn.in_proj_bias": (3 * d,),
                               p + "self_attn.out_proj.weight": (d, d), p + "self_attn.out_proj.bias": (d,),
                               p + "conv_module.layer_norm.weight": (d,), p + "conv_module.layer_norm.bias": (d,),
                               p + "conv_module.sequential.0.weight": (2 * d, d, 1), p + "conv_module.sequential.0.bias": (2 * d,),
                               p + "conv_module.sequential.2.weight": (d, 1, k), p + "conv_module.sequential.2.bias": (d,),
                               p + "conv_module.sequential.3.weight": (d,), p + "conv_module.sequential.3.bias": (d,),
                               p + "conv_module.sequential.3.running_mean": (d,), p + "conv_module.sequential.3.running_var": (d,),
                               p + "conv_module.sequential.5.weight": (d, d, 1), p + "conv_module.sequential.5.bias": (d,),
                               p + "final_layer_norm.weight": (d,), p + "final_layer_norm.bias": (d,)})
        vp = c.variance_predictors
        for name, cf in (("duration_predictor", vp.duration), ("pitch_predictor", vp.pitch), ("energy_predictor", vp.energy)):
            d, k = cf.input_dim, cf.kernel_size
            for i in range(cf.n_layers):
                p = f"{name}.convs.{i}"
                shapes.update({p + ".0.weight_g": (d, 1, 1), p + ".0.weight_v": (d, 1, k), p + ".0.bias": (d,),
                               p + ".1.weight_g": (d, 1, 1), p + ".1.weight_v": (d, d, 1), p + ".1.bias": (d,),
                               f"{name}.norms.{i}.weight": (d,), f"{name}.norms.{i}.bias": (d,)})
            shapes.update({name + ".linear.weight": (1, d), name + ".linear.bias": (1,)})
        d = c.encoder.input_dim
        if c.multispeaker:
            shapes["speaker_embedding.weight"] = (max(1, c.n_speakers), d)
        if c.multilingual:
            shapes["language_embedding.weight"] = (max(1, c.n_languages), d)
        if c.use_global_style_token_module:
            shapes.update(gst_state_dict_shapes(c))
        shapes.update({"pitch_embedding.weight": (vp.pitch.n_bins, d), "energy_embedding.weight": (vp.energy.n_bins, d),
                       "mel_linear.weight": (c.n_mels, c.decoder.input_dim), "mel_linear.bias": (c.n_mels,)})
        if c.use_postnet:
            dims = [c.n_mels] + [c.postnet_channels] * (c.postnet_layers - 1) + [c.n_mels]
            for i in range(c.postnet_layers):
                p = f"postnet.convolutions.{i}"
                shapes.update({p + ".0.weight": (dims[i + 1], dims[i], c.postnet_kernel), p + ".0.bias": (dims[i + 1],),
                               p + ".1.weight": (dims[i + 1],), p + ".1.bias": (dims[i + 1],),
                               p + ".1.running_mean": (dims[i + 1],), p + ".1.running_var": (dims[i + 1],)})
        return shapes

    def init_random(self, seed: int = 1234, aligner: bool = False):
        """Random parameters of the right shapes (benchmarks; there is no network for checkpoints).  ``aligner``: also the tensors of
        ``aligner_state_dict_shapes``, drawn after all the others (the model's own parameters do not depend on the flag)."""
        if aligner and not self.config.learn_alignment:
            raise ValueError("init_random(aligner=True): model.learn_alignment is off, this model has no aligner")
        g = torch.Generator().manual_seed(seed)
        sd = {}
        shapes = self.state_dict_shapes(self.config)
        if aligner:
            shapes.update(aligner_state_dict_shapes(self.config))
        for name, shape in shapes.items():
            if name.endswith("inv_freq"):
                d = self.config.encoder.input_dim
                sd[name] = 1.0 / (10000 ** (torch.arange(0.0, d, 2.0) / d))
            elif name.endswith("running_var") or name.endswith("weight_g") or (len(shape) == 1 and name.endswith(".weight")):
                sd[name] = torch.ones(shape)
            elif name.endswith("bias") or name.endswith("running_mean"):
                sd[name] = torch.zeros(shape)
            else:
                fan_in = max(1, int(torch.tensor(shape[1:]).prod())) if len(shape) > 1 else shape[0]
                sd[name] = torch.randn(shape, generator=g) / fan_in ** 0.5
        return self.load_state_dict(sd)

    # -- checkpoints (conventions of the reference: everyvoice/tests/test_model.py:85-151, 302-313, 454-459) -----------
    _VERSION = "1.0"

    def hyper_parameters(self) -> dict:
        from dataclasses import asdict
        return {"config": asdict(self.config), "stats": asdict(self.stats), "lang2id": dict(self.lang2id), "speaker2id": dict(self.speaker2id)}

    def to_checkpoint(self, state_dict: dict) -> dict:
        """Lightning-shaped dict: state_dict, JSON-only hyper_parameters (config, stats, lang2id, speaker2id), model_info."""
        return {"state_dict": {k: v.detach().cpu() for k, v in state_dict.items()}, "hyper_parameters": self.hyper_parameters(),
                "model_info": {"name": "FastSpeech2", "version": self._VERSION}}

    @classmethod
    def from_checkpoint(cls, ckpt: dict, device="cuda:0"):
        info = ckpt.get("model_info") if isinstance(ckpt, dict) else None
        if isinstance(info, dict) and info.get("name") != "FastSpeech2":
            raise TypeError(f"Wrong model type ({info.get('name')}), we are expecting a 'FastSpeech2' model")
        if isinstance(info, dict) and int(str(info.get("version", "1.0")).split(".")[0]) > int(cls._VERSION.split(".")[0]):
            raise ValueError("Your model was created with a newer version of EveryVoice, please update your software.")
        try:
            hp = ckpt["hyper_parameters"]
            c = hp["config"]
            cfg = FastSpeech2ModelConfig(
                encoder=ConformerConfig(**c["encoder"]), decoder=ConformerConfig(**c["decoder"]),
                variance_predictors=VariancePredictors(**{k: VariancePredictorConfig(**v) for k, v in c["variance_predictors"].items()}),
                **{k: v for k, v in c.items() if k not in ("encoder", "decoder", "variance_predictors")})
            stats = Stats(pitch=StatsInfo(**hp["stats"]["pitch"]), energy=StatsInfo(**hp["stats"]["energy"]))
        except (KeyError, TypeError) as e:
            raise TypeError("Unable to load config.  Possible causes: is it really a FastSpeech2Config? or the correct version?") from e
        model = cls(cfg, stats, device=device, lang2id=hp.get("lang2id"), speaker2id=hp.get("speaker2id"))
        return model.load_state_dict(ckpt["state_dict"])

    # -- forward --------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def __call__(self, ids: torch.Tensor, lens: torch.Tensor, duration_control=1.0, pitch_control=1.0, energy_control=1.0,
                 durations: torch.Tensor | None = None, speakers: torch.Tensor | None = None, languages: torch.Tensor | None = None,
                 style_mel: torch.Tensor | None = None, style_lens: torch.Tensor | None = None, pitch: torch.Tensor | None = None,
                 energy: torch.Tensor | None = None, target_frames: torch.Tensor | None = None):
        """ids [B, L] (0 = padding), lens [B] -> (mel [B, T, n_mels], postnet mel, durations [B, L], pitch, energy, mel_lens [B]) on the
        device.  ``pitch`` / ``energy`` (the predictions times their control, zero at padded positions) are [B, L] for a phone-level
        predictor and [B, T] for a frame-level one (``variance_predictors.<name>.level``).  ``style_mel`` (a model with the Global Style Token module needs it, any other
        refuses it): the style reference's mel [B, Ts, n_mels], or [1, Ts, n_mels] for one reference serving the whole batch.
        ``style_lens`` ([B] or [1], matching ``style_mel``): the references' frame counts; frames beyond them are absent (DESIGN.md
        section 25).  None: the references are consumed as given, padding included.

        Steering (refusals: ``check_prosody_arguments``).  Each ``*_control`` is a number for the whole batch, or a
        float tensor [B, L] (per symbol; values at padded symbols are ignored) or [B] (per item); a per-symbol control of a frame-level
        predictor follows its symbol through the length regulator.  ``pitch=`` / ``energy=`` force the embedded values, in the domain of
        the trainer's targets: [B, L] for a phone-level predictor, [B, T'] with T' at least the longest item's frames for a frame-level
        one; that predictor is not run, and the returned ``pitch`` / ``energy`` are the values that were embedded, zero at padding.
        ``target_frames`` (integer [B], 0 = no target): the item's mel has exactly that many frames, shared out over its symbols in
        proportion to the predicted durations times their controls (at most ``FIT_MAX_SYMBOLS`` symbols).  A negative target is refused
        where ``target_frames`` lives on the host; a tensor on the device is not synchronised with, and a target below 1 there means
        no target."""
        if not self._ready:
            raise RuntimeError("load_state_dict() or init_random() first")
        style_lens = check_style_lens(style_lens, None if style_mel is None else style_mel.shape)
        check_prosody_arguments(ids.shape[0], ids.shape[1], self.levels, duration_control, pitch_control, energy_control, pitch, energy,
                                target_frames, durations)
        with ops.mode(operands=self.precision):
            return self._forward(ids, lens, duration_control, pitch_control, energy_control, durations, speakers, languages, style_mel, style_lens,
                                 {"pitch": pitch, "energy": energy}, target_frames)

    def _text_embedding(self, ids, lens32, positional: bool):
        """ids [B, L] (or [B, L, 43] phonological feature vectors) -> [D, B, L], zero at the padded columns; ``positional``: plus the
        sinusoid (what the encoder reads; the aligner's keys are the embeddings alone)."""
        lib, dev, c = _lib.load(), self.device, self.config
        B, L = ids.shape[:2]
        D = c.encoder.input_dim
        if c.target_text_representation_level == "phonological_features":
            # Linear(43 -> D) as a pointwise convolution over [43, B, L]; the positional term also zeroes the padded columns
            if ids.dim() != 3 or ids.shape[2] != N_PHONOLOGICAL_FEATURES:
                raise ValueError(f"phonological features: expected [B, L, {N_PHONOLOGICAL_FEATURES}], got {tuple(ids.shape)}")
            feats = ids.to(dev, torch.float32).permute(2, 0, 1).contiguous()
            x = _conv(feats, self.table.view(D, N_PHONOLOGICAL_FEATURES, 1), None)
            if not positional:
                return _mask_cols_(x, lens32)
            _chk(lib.evmi_fs2_add_posemb_f32(x.data_ptr(), lens32.data_ptr(), self.inv_freq.data_ptr(), B, L, D, _s(x)), "evmi_fs2_add_posemb_f32")
            return x
        ids32 = ids.to(dev, torch.int32).contiguous()
        x = torch.empty(D, B, L, device=dev, dtype=torch.float32)
        _chk(lib.evmi_fs2_embed_f32(ids32.data_ptr(), lens32.data_ptr(), self.table.data_ptr(), self.inv_freq.data_ptr() if positional else 0,
                                    x.data_ptr(), B, L, D, _s(x)), "evmi_fs2_embed_f32")
        return x

    @torch.no_grad()
    def align(self, ids: torch.Tensor, lens: torch.Tensor, mel: torch.Tensor, mel_lens: torch.Tensor, speakers: torch.Tensor | None = None,
              languages: torch.Tensor | None = None, return_scores: bool = False, durations: torch.Tensor | None = None):
        """The durations [B, L] int64 (frames per symbol, zero at padded symbols; row b sums to mel_lens[b]) that the model's learnt
        aligner gives utterance b: ids [B, L], lens [B], its own mel [B, T, n_mels] and mel_lens [B].  What the trainer's aligner
        computes in a step, without the gradients' tensors: keys = the symbol embeddings (no positional term)
        through Conv(k 3) - ReLU - Conv(1), queries = the mel, zeroed at and beyond mel_lens, through Conv(k 3) - ReLU - Conv(1) - ReLU -
        Conv(1), both in fp32 in either precision mode; the beta-binomial prior of each item's (frames, symbols); the monotonic search
        over -temperature * ||q - k||^2 + log prior (``evmi_align_durations_f32``).  ``speakers`` / ``languages`` are accepted for symmetry
        with the forward and not used: the aligner reads the symbol embeddings alone.
        ``return_scores=True`` returns ``(durations, AlignmentScores(ctc, path, symbol))``: how well the aligner's soft attention agrees
        with those durations (``evmi_align_scores_f32``; float32 on the device) -- ctc [B], the CTC forward-sum loss
        of each utterance; path [B], its binarisation loss on the path of the durations; symbol [B, L], the mean log soft attention of
        each symbol over its own frames (0 at padded symbols).  ``durations=`` [B, L] of any integer type are scored in place of the
        search's, for alignments that come from elsewhere; they are returned as int64 on the device.  A row that does not give its
        lens[b] symbols mel_lens[b] frames in all is a ``ValueError`` where the tensor lives on the host, and NaN in ``path`` and
        ``symbol`` where it lives on the device (no transfer is made to look; an int64 entry beyond the int32 range is such a row too, it
        does not wrap); a symbol with no frame scores NaN.  ``ctc`` is the loss of the utterance aligned ALONE, over its own symbols:
        with the prior the trainer's value for the same utterance in a padded batch differs, because its first log-softmax runs over
        the padded symbols too.
        ``ValueError`` before any launch: a model without an aligner (``has_aligner``), ``mel`` not [B, T, n_mels], an item with fewer
        frames than symbols, ``durations`` without ``return_scores`` or not [B, L] integers."""
        if not self._ready:
            raise RuntimeError("load_state_dict() or init_random() first")
        c, dev = self.config, self.device
        if not self.has_aligner:
            raise ValueError("align: this model has no aligner (model.learn_alignment off, or the state dict held no `attention.*` tensors)")
        B, L = ids.shape[:2]
        if mel.dim() != 3 or mel.shape[0] != B or mel.shape[1] < 1 or mel.shape[2] != c.n_mels:
            raise ValueError(f"align: mel: expected [{B}, T, {c.n_mels}], got {tuple(mel.shape)}")
        T = mel.shape[1]
        n_sym, n_frm = [int(v) for v in lens.tolist()], [int(v) for v in mel_lens.tolist()]
        if len(n_sym) != B or len(n_frm) != B:
            raise ValueError(f"align: expected {B} lengths and {B} mel lengths, got {len(n_sym)} and {len(n_frm)}")
        for i in range(B):
            if not (1 <= n_sym[i] <= L and n_frm[i] <= T):
                raise ValueError(f"align: item {i}: {n_sym[i]} symbols of {L}, {n_frm[i]} frames of {T}")
            if n_frm[i] < n_sym[i]:
                raise ValueError(f"align: item {i} has {n_frm[i]} frames for {n_sym[i]} symbols: every symbol needs at least one frame")
        if durations is not None:
            if not return_scores:
                raise ValueError("align: durations= are scored, not searched: pass return_scores=True")
            if tuple(durations.shape) != (B, L) or durations.dtype not in (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64):
                raise ValueError(f"align: durations: expected [{B}, {L}] integers, got {tuple(durations.shape)} {durations.dtype}")
            if durations.device.type == "cpu":
                for i in range(B):
                    row = durations[i, : n_sym[i]].to(torch.int64)
                    if bool((row < 0).any()) or int(row.sum()) != n_frm[i]:
                        raise ValueError(f"align: durations: item {i}: the row gives its {n_sym[i]} symbols {int(row.sum())} frames "
                                         f"(least entry {int(row.min())}), the utterance has {n_frm[i]}")
        from .train.fs2 import _AlignerT

        q, k, prior, lens32, mel_lens32 = self._aligner_inputs(ids, mel, n_sym, n_frm)
        if not return_scores:
            return ops.align_durations(q, k, prior, lens32, mel_lens32, _AlignerT.temperature).to(torch.int64)
        if durations is None:
            dur32 = ops.align_durations(q, k, prior, lens32, mel_lens32, _AlignerT.temperature)
            dur64 = dur32.to(torch.int64)
        else:  # the kernel reads int32: an entry that does not fit there goes in as -1, which no valid row holds (NaN, as any negative entry)
            dur64 = durations.to(dev, torch.int64)
            dur32 = torch.where((dur64 >= 0) & (dur64 < 2 ** 31), dur64, -1).to(torch.int32).contiguous()
        scores = AlignmentScores(*ops.align_scores(q, k, prior, lens32, mel_lens32, dur32, _AlignerT.temperature))
        return dur64, scores

    def _aligner_inputs(self, ids, mel, n_sym, n_frm):
        """What both aligner kernels read, computed once: (q [A, B, T], k [A, B, L], prior [B, T, L] float64, lens32, mel_lens32) for
        ids [B, L], mel [B, T, n_mels] and the checked per-item symbol and frame counts."""
        from .heavy import BetaBinomialInterpolator

        c, dev = self.config, self.device
        (B, L), T = ids.shape[:2], mel.shape[1]
        lens32 = torch.tensor(n_sym, dtype=torch.int32, device=dev)
        mel_lens32 = torch.tensor(n_frm, dtype=torch.int32, device=dev)
        P = lambda name: (self.aligner[f"attention.{name}.conv.weight"], self.aligner[f"attention.{name}.conv.bias"])  # noqa: E731
        frames = torch.empty(c.n_mels, B, T, device=dev, dtype=torch.float32)
        frames.copy_(mel.to(dev).permute(2, 0, 1))
        _mask_cols_(frames, mel_lens32)
        with ops.exact_f32():
            k = ops.conv1d_fwd(self._text_embedding(ids, lens32, positional=False), *P("key_proj.0"), 1, 1, act=ops.ACT_RELU)
            k = ops.conv1d_fwd(k, *P("key_proj.2"))
            q = ops.conv1d_fwd(frames, *P("query_proj.0"), 1, 1, act=ops.ACT_RELU)
            q = ops.conv1d_fwd(ops.conv1d_fwd(q, *P("query_proj.2"), act=ops.ACT_RELU), *P("query_proj.4"))
        if getattr(self, "_prior", None) is None:
            self._prior = BetaBinomialInterpolator(device=dev)
        prior = torch.zeros(B, T, L, device=dev, dtype=torch.float64)
        for i in range(B):  # a function of (frames, symbols) alone: what the preprocessor's attn/ files hold
            prior[i, : n_frm[i], : n_sym[i]] = self._prior(n_frm[i], n_sym[i])
        return q, k, prior, lens32, mel_lens32

    def _forward(self, ids, lens, duration_control, pitch_control, energy_control, durations, speakers, languages, style_mel=None, style_lens=None,
                 forced=None, target_frames=None):
        lib, dev, c = _lib.load(), self.device, self.config
        B, L = ids.shape[:2]
        forced = {k: v for k, v in (forced or {}).items() if v is not None}

        def per_symbol(control):
            """A tensor control as float32 [B, L] on the device (a [B] one repeated along its row); None for a number."""
            if _is_scalar_control(control):
                return None
            t = control.to(dev, torch.float32)
            return (t[:, None].expand(B, L) if t.dim() == 1 else t).contiguous()
        if L > c.max_length:
            raise ValueError(f"text of {L} symbols exceeds max_length {c.max_length}")
        if self.gst is None and style_mel is not None:
            raise ValueError("`style_mel` given to a model without the Global Style Token module (model.use_global_style_token_module)")
        if self.gst is not None:
            if style_mel is None:
                raise ValueError("this model needs `style_mel` [B, Ts, n_mels]: it was trained with the Global Style Token module")
            if style_mel.dim() != 3 or style_mel.shape[0] not in (1, B) or style_mel.shape[1] < 1 or style_mel.shape[2] != c.n_mels:
                raise ValueError(f"style_mel: expected [{B} or 1, Ts, {c.n_mels}], got {tuple(style_mel.shape)}")
        D = c.encoder.input_dim
        lens32 = lens.to(dev, torch.int32).contiguous()
        x = self.encoder.forward(self._text_embedding(ids, lens32, positional=True), lens32)
        for table, item_ids, what in ((self.speaker_table, speakers, "speakers"), (self.language_table, languages, "languages")):
            if table is not None:
                if item_ids is None:
                    raise ValueError(f"this model needs `{what}` ids [B]")
                item32 = item_ids.to(dev, torch.int32).contiguous()
                _chk(lib.evmi_fs2_add_item_embedding_f32(x.data_ptr(), item32.data_ptr(), lens32.data_ptr(), table.data_ptr(), B, L, D, _s(x)),
                     "evmi_fs2_add_item_embedding_f32")
        if self.gst is not None:
            # the style matrix [B or 1, E] is the "table" of the same masked add; one reference: every item takes row 0 (computed once)
            style = self.gst.forward(style_mel.to(dev, torch.float32).contiguous(),
                                     None if style_lens is None else style_lens.to(dev, torch.int32).contiguous())
            rows = torch.arange(B, device=dev, dtype=torch.int32) if style.shape[0] == B else torch.zeros(B, device=dev, dtype=torch.int32)
            _chk(lib.evmi_fs2_add_item_embedding_f32(x.data_ptr(), rows.data_ptr(), lens32.data_ptr(), style.data_ptr(), B, L, D, _s(x)),
                 "evmi_fs2_add_item_embedding_f32")
        log_d = self.duration_predictor.forward(x, lens32)
        vp = c.variance_predictors
        variances = (("pitch", self.pitch_predictor, self.pitch_bins, self.pitch_table, vp.pitch.n_bins, pitch_control),
                     ("energy", self.energy_predictor, self.energy_bins, self.energy_table, vp.energy.n_bins, energy_control))
        out, steered = {}, {}  # steered[name]: the embedded values as the steered kernel wrote them (what the call returns for that variance)

        def adapt(level, h, h_lens, n, cum=None):
            """pitch, then energy, for the predictors of this level: predict on h [D, B, n], add the bucket embedding of prediction * control
            in place (at padded positions too: the value there is 0, and the next predictor's k = 3 convolutions see those columns).
            A forced variance or a tensor control goes through evmi_fs2_variance_apply_f32 (``cum``: the frame axis, where a control
            follows its symbol), everything else through the call it always went through."""
            for name, pred, bins, table, n_bins, control in variances:
                if self.levels[name] != level:
                    continue
                values, ctl = forced.get(name), per_symbol(control)
                if values is None and ctl is None:
                    out[name] = pred.forward(h, h_lens)
                    _chk(lib.evmi_fs2_bucket_embed_add_f32(h.data_ptr(), out[name].data_ptr(), bins.data_ptr(), table.data_ptr(), n_bins, B, n, D,
                                                           float(control), _s(h)), "evmi_fs2_bucket_embed_add_f32")
                    continue
                if values is not None:
                    values, p = values.to(dev, torch.float32).contiguous(), None
                else:
                    p = pred.forward(h, h_lens)
                steered[name] = out[name] = torch.empty(B, n, device=dev, dtype=torch.float32)
                _chk(lib.evmi_fs2_variance_apply_f32(h.data_ptr(), _lib.ptr(p), _lib.ptr(values), 0 if values is None else values.shape[1],
                                                     _lib.ptr(ctl), _lib.ptr(cum if ctl is not None else None), h_lens.data_ptr(), bins.data_ptr(),
                                                     table.data_ptr(), out[name].data_ptr(), n_bins, B, L if cum is not None and ctl is not None else n,
                                                     n, D, 1.0, _s(h)), "evmi_fs2_variance_apply_f32")

        adapt("phone", x, lens32, L)
        dur_ctl = per_symbol(duration_control)
        if durations is None and (dur_ctl is not None or target_frames is not None):
            dur = torch.empty(B, L, device=dev, dtype=torch.int32)
            weights = torch.empty(B, L, device=dev, dtype=torch.float32) if target_frames is not None else None
            _chk(lib.evmi_fs2_durations_ctl_i32(log_d.data_ptr(), lens32.data_ptr(), _lib.ptr(dur_ctl), dur.data_ptr(), _lib.ptr(weights), B, L,
                                                1.0 if dur_ctl is not None else float(duration_control), _s(x)), "evmi_fs2_durations_ctl_i32")
            if target_frames is not None:
                target32 = target_frames.to(dev, torch.int32).contiguous()
                _chk(lib.evmi_fs2_fit_durations_i32(weights.data_ptr(), lens32.data_ptr(), target32.data_ptr(), dur.data_ptr(), B, L, _s(x)),
                     "evmi_fs2_fit_durations_i32")
        elif durations is None:
            dur = torch.empty(B, L, device=dev, dtype=torch.int32)
            _chk(lib.evmi_fs2_durations_i32(log_d.data_ptr(), lens32.data_ptr(), dur.data_ptr(), B, L, float(duration_control), _s(x)),
                 "evmi_fs2_durations_i32")
        else:
            pad = torch.arange(L, device=dev)[None, :] >= lens32[:, None]
            dur = durations.to(dev, torch.int32).clamp_min(0).masked_fill(pad, 0).contiguous()
        cum = torch.cumsum(dur, 1, dtype=torch.int32).contiguous()
        mel_lens = cum[:, -1].contiguous()
        T = int(mel_lens.max())  # the one host sync of the forward: the output length (in front of every frame-level predictor)
        if T <= 0:
            raise ValueError("all predicted durations are zero")
        for name, values in forced.items():  # (a frame-level tensor can be held to T only here; phone level was checked before any launch)
            if self.levels[name] == "frame" and values.shape[1] < T:
                raise ValueError(f"{name}: forced values [{B}, {values.shape[1]}] are shorter than the longest item's {T} frames")
        frames = torch.empty(D, B, T, device=dev, dtype=torch.float32)
        _chk(lib.evmi_length_regulate_cbt_f32(x.data_ptr(), cum.data_ptr(), frames.data_ptr(), D, B, L, T, _s(x)), "evmi_length_regulate_cbt_f32")
        adapt("frame", frames, mel_lens, T, cum)
        pitch, energy = out["pitch"], out["energy"]
        _chk(lib.evmi_fs2_add_posemb_f32(frames.data_ptr(), mel_lens.data_ptr(), self.inv_freq.data_ptr(), B, T, D, _s(x)), "evmi_fs2_add_posemb_f32")
        y = self.decoder.forward(frames, mel_lens)
        mel = _conv(y, self.w_mel, self.b_mel)
        _chk(lib.evmi_mask_cols_f32(mel.data_ptr(), mel_lens.data_ptr(), c.n_mels, B, T, _s(x)), "evmi_mask_cols_f32")
        post = mel
        if self.postnet:
            h = mel
            for i, (w, b) in enumerate(self.postnet):
                if c.mask_padding and i > 0:  # tanh(bias) beyond the length (layer 0 reads the masked mel): postnet_layers - 1 launches
                    _mask_cols_(h, mel_lens)
                h = _conv(h, w, b, c.postnet_kernel, act=ops.ACT_TANH if i < len(self.postnet) - 1 else ops.ACT_NONE)
            post = ops.axpby(1.0, mel, 1.0, h)
            _chk(lib.evmi_mask_cols_f32(post.data_ptr(), mel_lens.data_ptr(), c.n_mels, B, T, _s(x)), "evmi_mask_cols_f32")
        to_btc = lambda t: t.permute(1, 2, 0).contiguous()
        mult = lambda name, v, s: v if name in steered or s == 1.0 else v * s
        return (to_btc(mel), to_btc(post), dur.to(torch.int64), mult("pitch", pitch, pitch_control), mult("energy", energy, energy_control),
                mel_lens.to(torch.int64))

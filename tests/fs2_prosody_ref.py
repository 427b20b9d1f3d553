"""torch-CPU restatement of FastSpeech2's prosody steering -- a test helper beside the oracle, like
``tests/fs2_levels_ref.py``, from whose pieces (and so from the modules of ``oracle.fs2_ref.FastSpeech2Ref``) it is composed:

  * ``fit_ref``: the largest-remainder apportionment of a number of frames over weights, in Python floats (= doubles);
  * ``forward_prosody_ref``: the inference forward with a control per symbol ([B, L], or [B], or a number) for the durations and
    either variance at either level, forced pitch / energy values, and given durations;
  * ``fit_shares_ref``: the float64 shares x_l that ``target_frames`` apportions.
"""

import math

import torch

from oracle.heavy_ref import expand_ref
from tests.fs2_levels_ref import _encode, _levels, _variance

MARGIN = 1e-3


def fit_ref(weights, target: int, current=None):
    """-> the durations (a list of ints) of ``target`` frames over ``weights`` (floats; all zero = all equal): x_l = w_l * target / S,
    floor, and the target - sum floor symbols with the largest remainder get one frame more, ties to the lower index.  ``target`` <= 0:
    ``current`` is returned as it is."""
    if target <= 0:
        return list(current) if current is not None else None
    w = [float(v) if v > 0 else 0.0 for v in weights]
    S = math.fsum(w)  # (exact on the lattice the tests use; on any other input only invariants are compared)
    if S == 0.0:
        w, S = [1.0] * len(w), float(len(w))
    x = [(v * target) / S for v in w]
    q = [math.floor(v) for v in x]
    R = target - sum(q)
    assert 0 <= R <= len(w), (R, len(w))
    order = sorted(range(len(w)), key=lambda i: (-(x[i] - q[i]), i))
    for i in order[:R]:
        q[i] += 1
    return [int(v) for v in q]


def per_symbol(control, B, L):
    """A control as the product takes it -> float32 [B, L]."""
    if not isinstance(control, torch.Tensor):
        return torch.full((B, L), float(control), dtype=torch.float32)
    t = control.to(torch.float32)
    return t[:, None].expand(B, L).contiguous() if t.dim() == 1 else t


def symbol_of_frame(durations, T):
    """[B, T]: the symbol the length regulator puts at frame t = the first l with cum[b][l] > t (L - 1 past the item's frames)."""
    cum = torch.cumsum(durations, 1)
    t = torch.arange(T)[None, :].expand(durations.shape[0], T).contiguous()
    return torch.searchsorted(cum, t, right=True).clamp_max(durations.shape[1] - 1)


@torch.no_grad()
def fit_shares_ref(model, ids, lens, duration_control, target_frames, guard=True):
    """float64 [B, L]: the shares x_l = w_l * target / S with w_l = max(0, (exp(log_d) - 1) * control) from the oracle's log-durations
    (zero at padded symbols and for items without a target).  ``guard``: assert that no share of an item with a target sits within 1e-3
    of a whole number: a fit gives every symbol floor(x_l) or floor(x_l) + 1 frames, so a device whose log-durations differ from the
    oracle's in the last bits stays strictly within one frame of the oracle's x_l as long as its own share has the same floor
    ("pick another seed" otherwise)."""
    B, L = ids.shape
    x, pad = _encode(model, ids, lens, None, None)
    log_d = model.duration_predictor(x, pad).double()
    w = ((torch.exp(log_d) - 1.0) * per_symbol(duration_control, B, L).double()).clamp_min(0.0).masked_fill(pad, 0.0)
    S = w.sum(1, keepdim=True)
    assert bool((S > 0).all())
    shares = w * target_frames.double()[:, None] / S
    if guard:
        frac = shares - torch.floor(shares)
        inside = (frac > MARGIN) & (frac < 1.0 - MARGIN)
        assert bool((inside | pad | (target_frames <= 0)[:, None]).all()), "a share sits on a whole number of frames: pick another seed"
    return shares


@torch.no_grad()
def forward_prosody_ref(model, ids, lens, duration_control=1.0, pitch_control=1.0, energy_control=1.0, durations=None, pitch=None,
                        energy=None, guard=True):
    """-> (mel, postnet mel, durations, pitch, energy, mel_lens), pitch / energy = the embedded values ([B, T] for a frame-level
    predictor), zero at padding.  ``guard``: assert that no predicted duration sits within 1e-3 of a rounding boundary and no
    PREDICTED value times its control within 1e-3 of a bin edge (forced values are the same numbers on both sides)."""
    B, L = ids.shape[:2]
    levels = _levels(model)
    controls = {"pitch": per_symbol(pitch_control, B, L), "energy": per_symbol(energy_control, B, L)}
    forced = {"pitch": pitch, "energy": energy}
    x, pad = _encode(model, ids, lens, None, None)
    log_d = model.duration_predictor(x, pad)
    out = {}

    def value(name, h, hpad, control):
        predictor, embedding, bins = _variance(model, name)
        if forced[name] is not None:
            v = forced[name][:, : h.shape[1]].to(torch.float32).masked_fill(hpad, 0.0)
        else:
            v = (predictor(h, hpad) * control).masked_fill(hpad, 0.0)
            if guard:
                edge = (v[..., None] - bins).abs().min(-1).values
                assert bool(((edge > MARGIN) | hpad).all()), f"a predicted {name} value sits on a bin edge: pick another seed"
        out[name] = v
        return h + embedding(torch.bucketize(v, bins))

    for name in ("pitch", "energy"):
        if levels[name] == "phone":
            x = value(name, x, pad, controls[name])
    if durations is None:
        raw = torch.exp(log_d) - 1.0
        if guard:
            assert bool((((raw - torch.floor(raw) - 0.5).abs() > MARGIN) | pad).all()), "test input sits on a rounding boundary: pick another seed"
        durations = torch.clamp(torch.round(raw) * per_symbol(duration_control, B, L), min=0).long()
    durations = durations.masked_fill(pad, 0)
    mel_lens = durations.sum(1)
    T = int(mel_lens.max())
    frames = torch.zeros(B, T, x.shape[2])
    for b in range(B):
        e = torch.from_numpy(expand_ref(x[b].numpy(), durations[b].numpy()))
        frames[b, : e.shape[0]] = e
    fpad = torch.arange(T)[None, :] >= mel_lens[:, None]
    sym = symbol_of_frame(durations, T)
    for name in ("pitch", "energy"):
        if levels[name] == "frame":
            frames = value(name, frames, fpad, torch.gather(controls[name], 1, sym))
    y = (frames + model.position_embedding(T)[None]).masked_fill(fpad[..., None], 0.0)
    y, _ = model.decoder(y, mel_lens)
    mel = model.mel_linear(y).masked_fill(fpad[..., None], 0.0)
    post = mel + model.postnet(mel) if model.postnet is not None else mel
    post = post.masked_fill(fpad[..., None], 0.0)
    return mel, post, durations, out["pitch"], out["energy"], mel_lens

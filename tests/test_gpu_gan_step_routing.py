"""Which discriminator chain of a GAN step runs on which stream, in which host order (train/hifigan.py: ``g_step_routing`` for the
generator step, ``_DiscFacts.slot`` for the discriminator step), read off one eager step on the GPU.  The streams matter because the
per-stream workspaces grown by the eager warm-up steps are the ones a captured graph uses.  Default model: 5 period discriminators
(0..4), 3 scale discriminators (5..7), the first of them spectral-norm."""

import pytest
import torch

pytestmark = pytest.mark.gpu

SN = 5  # the spectral-norm scale


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_every_chain_of_a_step_runs_on_its_stream_in_its_host_order(cuda_device, precision):
    from everyvoice_amd.train.hifigan import HiFiGANTrainer

    g = torch.Generator().manual_seed(8)
    B, S = 2, 2048
    y = (0.3 * torch.tanh(torch.randn(B, 1, S, generator=g))).to(cuda_device)
    mel = torch.randn(B, 80, S // 256, generator=g).to(cuda_device)
    tr = HiFiGANTrainer(device=cuda_device, seed=5, precision=precision, use_graph=False)
    log = []

    def logged(i, d):
        forward = d.forward

        def wrapper(tape, x, training=True, role="pair", grad_from=None):
            log.append((i, role, torch.cuda.current_stream(cuda_device)))
            return forward(tape, x, training, role, grad_from)

        return wrapper

    for i, d in enumerate(tr.discriminators()):
        d.forward = logged(i, d)
    recon_grad = tr._recon_grad

    def recon(*args):
        log.append((None, "recon", torch.cuda.current_stream(cuda_device)))
        return recon_grad(*args)

    tr._recon_grad = recon
    tr.training_step(mel, y)
    streams = tr.branches.streams
    assert len(streams) == 18

    # discriminator step: every chain on its slot; the spectral-norm scale's two calls on 5 and 6, the pooled scales on 7 and 8
    d_step = [e for e in log if e[1] in ("pair", "real", "fake")]
    want = [(i, "pair", streams[i]) for i in range(5)] + [(SN, "real", streams[5]), (SN, "fake", streams[6]), (6, "pair", streams[7]), (7, "pair", streams[8])]
    assert d_step == want

    # generator step: exactly the chains of the routing table, each on the stream of its branch, issued in the table's host order
    g_step = [e for e in log if e[1] not in ("pair", "real", "fake")]
    if precision == "f32":  # two calls per discriminator: generated chains on 0..7, real chains on 8..15, the reconstruction loss on 16
        table = [(i, "g_fake", i) for i in range(8)] + [(i, "g_real", 8 + i) for i in range(8)] + [(None, "recon", 16)]
        order = [8 + SN] + [j for j in range(17) if j != 8 + SN]
        assert sum(e[1] == "g_fake" for e in g_step) == 8 and sum(e[1] == "g_real" for e in g_step) == 8
    else:  # packed chains: [real | generated] as one batch, but for the spectral-norm scale (its real chain on 8); reconstruction on 9
        table = [(i, "g_fake" if i == SN else "g_both", i) for i in range(8)] + [(SN, "g_real", 8), (None, "recon", 9)]
        order = [8, 0, 1, 2, 3, 4, 5, 6, 7, 9]
        assert sum(e[1] == "g_both" for e in g_step) == 7 and [e[1] for e in g_step if e[0] == SN] == ["g_real", "g_fake"]
    assert g_step == [(table[j][0], table[j][1], streams[table[j][2]]) for j in order]
    roles = [(i, role) for i, role, _ in g_step]
    assert roles.index((SN, "g_real")) < roles.index((SN, "g_fake"))  # the real call takes the first prepared spectral-norm weights

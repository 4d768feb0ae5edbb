"""CPU tests of CFM.forward / CFM.flow_loss (the flow-matching loss, forward only) over the oracle backbone: the host logic and the order of its
random draws against vectors the reference's own CFM.forward produced (tools/make_cfm_forward_golden.py -> tests/golden/cfm_forward.npz),
mask_from_frac_lengths against the reference's, injected draws, and eval.validate.validation_loss."""
import math
import random

import pytest
import torch

from conftest import golden_arch, golden_weights, load_golden, rel_l2


class _Backbone(torch.nn.Module):
    """plug point A over the CPU oracle on the tiny_base network; keeps the keyword arguments of every call."""

    def __init__(self):
        super().__init__()
        from oracle import cpu_ref
        z = load_golden("tiny_base")
        self.W, self.cfg, self.ref, self.dim = golden_weights(z), golden_arch(z), cpu_ref, golden_arch(z)["dim"]
        self.p = torch.nn.Parameter(torch.zeros(1))
        self.calls = []

    def forward(self, **kw):
        self.calls.append(kw)
        assert set(kw) == {"x", "cond", "text", "time", "drop_audio_cond", "drop_text"}, sorted(kw)  # cfm.py:275-277: no mask, no cache
        return self.ref.dit_forward(self.W, self.cfg, kw["x"], kw["cond"], kw["text"], kw["time"], kw["drop_audio_cond"], kw["drop_text"])


@pytest.fixture(scope="module")
def golden():
    return load_golden("cfm_forward")


@pytest.fixture(scope="module")
def cfm():
    from eraxvif5tts_amd.model import CFM
    return CFM(transformer=_Backbone(), mel_spec_kwargs={"mel_spec_type": "vocos"})


def _inputs(z):
    return torch.from_numpy(z["mel"]), torch.from_numpy(z["text"]), torch.from_numpy(z["lens"])


def test_golden_covers_both_drop_branches(golden):
    flags = {tuple(bool(v) for v in golden[f"s{s}.flags"]) for s in golden["seeds"]}
    assert {(False, False), (True, True)} <= flags


def test_forward_matches_the_reference(golden, cfm):
    """The reference's CFM.forward after torch.manual_seed(s); random.seed(s): cond bit for bit (the span comes from the first two torch draws),
    the drop flags (the two random() calls), pred and loss to the tolerance of test_cfm_host_logic_against_reference_golden (x0 and time, the
    third and fourth torch draws, enter pred through phi)."""
    mel, text, lens = _inputs(golden)
    for s in golden["seeds"]:
        torch.manual_seed(int(s))
        random.seed(int(s))
        loss, cond, pred = cfm(mel, text, lens=lens)
        assert torch.equal(cond, torch.from_numpy(golden[f"s{s}.cond"])), s
        kw = cfm.transformer.calls[-1]
        assert (kw["drop_audio_cond"], kw["drop_text"]) == tuple(bool(v) for v in golden[f"s{s}.flags"]), s
        assert rel_l2(pred, golden[f"s{s}.pred"]) < 2e-5, s
        assert abs(float(loss) - float(golden[f"s{s}.loss"])) < 2e-5 * abs(float(golden[f"s{s}.loss"])), s
        assert not pred.requires_grad and not loss.requires_grad


def test_flow_loss_fields_are_consistent(golden, cfm):
    mel, text, lens = _inputs(golden)
    s = int(golden["seeds"][0])
    torch.manual_seed(s)
    random.seed(s)
    r = cfm.flow_loss(mel, text, lens=lens)
    assert torch.equal(r.rand_span_mask, torch.from_numpy(golden[f"s{s}.span"]))
    assert r.sums.dtype == torch.float64 and r.counts.dtype == torch.int64
    assert torch.equal(r.counts, r.rand_span_mask.sum(dim=1) * mel.shape[-1])
    elem = (r.pred - (mel - r.x0)) ** 2
    for b in range(mel.shape[0]):
        want = float(elem[b][r.rand_span_mask[b]].double().sum())
        assert abs(float(r.sums[b]) - want) <= 1e-12 * want
    assert abs(float(r.loss) - float(r.sums.sum()) / int(r.counts.sum())) <= 2.0 ** -22 * float(r.loss)
    assert torch.equal(r.cond, torch.where(r.rand_span_mask[..., None], torch.zeros_like(mel), mel))
    # the same draws handed back in: nothing is drawn, and the result is the same
    state, pstate = torch.get_rng_state(), random.getstate()
    again = cfm.flow_loss(mel, text, lens=lens, x0=r.x0, time=r.time, rand_span_mask=r.rand_span_mask, drop_audio_cond=r.drop_audio_cond,
                          drop_text=r.drop_text)
    assert torch.equal(torch.get_rng_state(), state) and random.getstate() == pstate
    assert torch.equal(again.pred, r.pred) and torch.equal(again.loss, r.loss) and torch.equal(again.sums, r.sums)


def test_mask_from_frac_lengths_matches_the_reference(golden):
    from eraxvif5tts_amd.model.utils import mask_from_frac_lengths, mask_from_start_end_indices
    seq_len, frac = torch.from_numpy(golden["frac.seq_len"]), torch.from_numpy(golden["frac.frac"])
    assert float(frac.min()) == pytest.approx(0.7) and float(frac.max()) == 1.0  # both ends of CFM's (0.7, 1.0)
    for s in (0, 1, 2):
        torch.manual_seed(s)
        got = mask_from_frac_lengths(seq_len, frac)
        assert torch.equal(got, torch.from_numpy(golden[f"frac.mask{s}"])), s
        assert torch.equal(torch.rand(4), torch.from_numpy(golden[f"frac.next{s}"])), s  # one rand_like draw, no more
        lengths = (frac * seq_len).long()
        assert torch.equal(got.sum(dim=1), lengths)  # the span holds the truncated product; a full fraction selects every frame
    m = mask_from_start_end_indices(torch.tensor([5, 3]), torch.tensor([1, 0]), torch.tensor([4, 9]))
    assert m.tolist() == [[False, True, True, True, False], [True] * 5]


def test_injected_draws_are_honoured_and_the_rest_keep_their_order(golden, cfm):
    mel, text, lens = _inputs(golden)
    B = mel.shape[0]
    g = torch.Generator().manual_seed(99)
    x0 = torch.randn(mel.shape, generator=g)
    time = torch.tensor([0.0, 1.0, 0.25])

    # the reference's stream: uniform_ [B], rand_like [B], randn_like(x1), rand((B,)), random(), random()
    def stream(seed, skip=()):
        torch.manual_seed(seed)
        random.seed(seed)
        d = {}
        if "span" not in skip:
            d["frac"] = torch.zeros((B,)).float().uniform_(0.7, 1.0)
            d["start"] = torch.rand_like(d["frac"])
        if "x0" not in skip:
            d["x0"] = torch.randn_like(mel)
        if "time" not in skip:
            d["time"] = torch.rand((B,))
        d["r1"] = None if "audio" in skip else random.random()
        d["r2"] = None if "text" in skip else random.random()
        return d

    def run(seed, **kw):
        torch.manual_seed(seed)
        random.seed(seed)
        return cfm.flow_loss(mel, text, lens=lens, **kw)

    base, d = run(7), stream(7)
    assert torch.equal(base.x0, d["x0"]) and torch.equal(base.time, d["time"])
    assert base.drop_text == (d["r2"] < cfm.cond_drop_prob) and base.drop_audio_cond == (d["r1"] < cfm.audio_drop_prob or base.drop_text)

    r, d = run(7, x0=x0), stream(7, skip=("x0",))
    assert torch.equal(r.x0, x0) and torch.equal(r.time, d["time"]) and torch.equal(r.rand_span_mask, base.rand_span_mask)
    r, d = run(7, time=time), stream(7, skip=("time",))
    assert torch.equal(r.time, time) and torch.equal(r.x0, d["x0"])
    # t = 0 and t = 1: phi is the noise / the mel itself
    x = cfm.transformer.calls[-1]["x"]
    assert torch.equal(x[0], r.x0[0]) and torch.equal(x[1], mel[1])
    span = torch.zeros(mel.shape[:2], dtype=torch.bool)
    span[:, 3:9] = True
    r, d = run(7, rand_span_mask=span), stream(7, skip=("span",))
    assert torch.equal(r.rand_span_mask, span) and torch.equal(r.x0, d["x0"]) and torch.equal(r.time, d["time"])
    assert torch.equal(r.counts, torch.full((B,), 6 * mel.shape[-1]))
    # a given flag skips its random() call; the other call is the next number of the stream
    r, d = run(7, drop_audio_cond=False), stream(7, skip=("audio",))
    assert r.drop_audio_cond is False and r.drop_text == (d["r2"] < cfm.cond_drop_prob)
    for flags in ((False, False), (True, True), (True, False), (False, True)):
        r = run(7, drop_audio_cond=flags[0], drop_text=flags[1])
        kw = cfm.transformer.calls[-1]
        assert (r.drop_audio_cond, r.drop_text) == flags == (kw["drop_audio_cond"], kw["drop_text"])
    random.seed(7)
    want = random.getstate()
    r = run(7, drop_audio_cond=True, drop_text=False)
    assert random.getstate() == want  # neither random() call was made


def test_empty_span_gives_nan_and_zero_counts(golden, cfm):
    mel, text, lens = _inputs(golden)
    r = cfm.flow_loss(mel, text, lens=lens, rand_span_mask=torch.zeros(mel.shape[:2], dtype=torch.bool), drop_audio_cond=False, drop_text=False)
    assert math.isnan(float(r.loss)) and r.counts.tolist() == [0, 0, 0] and r.sums.tolist() == [0.0, 0.0, 0.0]
    assert torch.equal(r.cond, mel)


def test_validation_loss_is_reproducible_and_adds_up(golden, cfm):
    from eraxvif5tts_amd.eval import validation_loss
    mel, text, lens = _inputs(golden)
    batches = [(mel, text, lens), (mel[:2, :22], text[:2], torch.tensor([22, 15]))]
    a = validation_loss(cfm, batches, seed=3)
    b = validation_loss(cfm, batches, seed=3)
    assert a.loss == b.loss and a.utterance_losses == b.utterance_losses and torch.equal(a.sums, b.sums)
    assert len(a.utterance_losses) == 5 and a.frames * mel.shape[-1] == int(a.counts.sum())
    parts = []
    for i, (m, t, n) in enumerate(batches):
        torch.manual_seed(3 + i)
        random.seed(3 + i)
        parts.append(cfm.flow_loss(m, t, lens=n, drop_audio_cond=False, drop_text=False))
    assert torch.equal(a.sums, torch.cat([p.sums for p in parts])) and torch.equal(a.counts, torch.cat([p.counts for p in parts]))
    assert a.loss == math.fsum(torch.cat([p.sums for p in parts]).tolist()) / int(torch.cat([p.counts for p in parts]).sum())
    assert validation_loss(cfm, batches, seed=4).loss != a.loss
    kw = cfm.transformer.calls[-1]
    assert kw["drop_audio_cond"] is False and kw["drop_text"] is False

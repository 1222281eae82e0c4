"""Pin the CPU oracle against golden vectors produced by the reference itself (CPU only).

Tolerance: max|a-b| / max|b| <= 1e-4 (fp32; BASELINE north_star); the oracle
restates the same torch CPU arithmetic, so it lands near 1e-6.
"""
import numpy as np
import pytest
import torch

from oracle import mrg_oracle as O
from tests.golden_util import load, config, batch_from, prefixed, rel_err

TOL = 1e-4


def test_attention_masks_match_reference():
    d = load("attention_masks")
    for i in range(5):
        main = torch.from_numpy(d[f"case{i}/main"])
        other = torch.from_numpy(d[f"case{i}/other"])
        heads = int(d[f"case{i}/heads"])
        got = O.gen_attention_mask(main, other, heads)
        assert torch.equal(got, torch.from_numpy(d[f"case{i}/mask"])), i


def test_mask_rejects_non_divisible():
    with pytest.raises(ValueError):
        O.gen_attention_mask(torch.zeros(1, 4, 2), torch.zeros(1, 6, 2), 1)


def test_lstm_layer_matches_nn_lstm_golden():
    d = load("ops")
    p = prefixed(d, "lstm1/param/")
    x = torch.from_numpy(d["lstm1/x"]).requires_grad_(True)
    h0 = torch.from_numpy(d["lstm1/h0"])[0].clone().requires_grad_(True)
    c0 = torch.from_numpy(d["lstm1/c0"])[0].clone().requires_grad_(True)
    w = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    y, hT, cT = O.lstm_layer(x, w["weight_ih_l0"], w["weight_hh_l0"], w["bias_ih_l0"], w["bias_hh_l0"], h0, c0)
    assert rel_err(y, d["lstm1/y"]) < TOL
    assert rel_err(hT, d["lstm1/hT"][0]) < TOL
    assert rel_err(cT, d["lstm1/cT"][0]) < TOL
    loss = (y * torch.from_numpy(d["lstm1/dy"])).sum() + (hT * torch.from_numpy(d["lstm1/dhT"])[0]).sum() \
        + (cT * torch.from_numpy(d["lstm1/dcT"])[0]).sum()
    loss.backward()
    assert rel_err(x.grad, d["lstm1/dx"]) < TOL
    assert rel_err(h0.grad, d["lstm1/dh0"][0]) < TOL
    assert rel_err(c0.grad, d["lstm1/dc0"][0]) < TOL
    for k in w:
        assert rel_err(w[k].grad, d[f"lstm1/grad/{k}"]) < TOL, k


def test_bidirectional_two_layer_lstm_golden():
    d = load("ops")
    sd = {k: v.clone().requires_grad_(True) for k, v in prefixed(d, "lstm2/param/").items()}
    x = torch.from_numpy(d["lstm2/x"]).requires_grad_(True)
    y, (hT, cT) = O.lstm_stack(x, sd, "", 2, True)
    assert rel_err(y, d["lstm2/y"]) < TOL
    assert rel_err(hT, d["lstm2/hT"]) < TOL
    assert rel_err(cT, d["lstm2/cT"]) < TOL
    (y * torch.from_numpy(d["lstm2/dy"])).sum().backward()
    assert rel_err(x.grad, d["lstm2/dx"]) < TOL
    for k in sd:
        assert rel_err(sd[k].grad, d[f"lstm2/grad/{k}"]) < TOL, k


@pytest.mark.parametrize("case", [0, 1, 2])
def test_mha_with_reference_mask_golden(case):
    d = load("ops")
    p = f"mha{case}/"
    sd = {k: v.clone().requires_grad_(True) for k, v in prefixed(d, p + "param/").items()}
    q = torch.from_numpy(d[p + "q"]).requires_grad_(True)
    kv = torch.from_numpy(d[p + "kv"]).requires_grad_(True)
    mask = torch.from_numpy(d[p + "mask"])
    o = O.mha(q, kv, sd, "", int(d[p + "heads"]), mask)
    assert rel_err(o, d[p + "o"]) < TOL
    (o * torch.from_numpy(d[p + "do"])).sum().backward()
    assert rel_err(q.grad, d[p + "dq"]) < TOL
    assert rel_err(kv.grad, d[p + "dkv"]) < TOL
    for k in sd:
        assert rel_err(sd[k].grad, d[p + f"grad/{k}"]) < TOL, k


def test_adamw_restatement_matches_reference_step():
    d = load("metaformer_small_r1")
    params = {k[6:]: torch.from_numpy(d[k]).clone() for k in d.files if k.startswith("param/")}
    grads = {k: torch.from_numpy(d["grad/" + k]) for k in params}
    cfg = config(d)["optim"]
    O.adamw_step(params, grads, {}, cfg["lr"], cfg["weight_decay"])
    for k, v in params.items():
        assert rel_err(v, d["after/" + k]) < 1e-6, k


def _check_train(d, loss, y, grads, after, y_key="y", check_y=True):
    assert abs(loss.item() - float(d["loss"])) / abs(float(d["loss"])) < TOL
    if check_y:
        assert rel_err(y, d[y_key]) < TOL
    for k, g in grads.items():
        if f"grad/{k}" in d.files:
            assert rel_err(g, d[f"grad/{k}"]) < TOL, k
        elif f"gradsum/{k}" in d.files:
            ref = d[f"gradsum/{k}"]
            gg = g.double()
            assert abs(gg.sum().item() - ref[0]) <= TOL * max(abs(ref[0]), np.sqrt(ref[1]), 1e-6), k
            assert abs((gg ** 2).sum().item() - ref[1]) <= 1e-3 * max(ref[1], 1e-12), k
        if f"after/{k}" in d.files:
            # Adam's first step is ~ -lr*sign(g): compare where the reference gradient is
            # above fp32 noise (zero-gradient entries, e.g. the MHA key bias, have random sign; the
            # 1e-6 floor is the GPU tests' _check_after rule: the key-bias third of in_proj_bias has an
            # analytically zero gradient whose fp32 noise can exceed 1e-5 of the tensor's max)
            gref = torch.from_numpy(d[f"grad/{k}"])
            sel = gref.abs() > torch.clamp(1e-5 * gref.abs().max(), min=1e-6)
            if sel.any():
                assert rel_err(after[k][sel], torch.from_numpy(d[f"after/{k}"])[sel]) < TOL, k


@pytest.mark.parametrize("name", ["metaformer_small_r1", "metaformer_small_r2_pad", "metaformer_gru_r2_pad"])
def test_metaformer_small_train_step(name):
    d = load(name)
    cfg = config(d)
    sd = prefixed(d, "param/")
    batch = batch_from(d)
    with torch.no_grad():
        inp = list(batch[:-1])
        ms = inp[2][0]
        inp[2] = (ms * (ms != -100).int(), inp[2][1])
        assert rel_err(O.metaformer_forward(sd, cfg["model"], inp), d["y"]) < TOL
        assert rel_err(O.metaformer_forward(sd, cfg["model"], batch[:-1]), d["y_eval"]) < TOL
    loss, y, grads, after = O.run_train_step(O.metaformer_training_loss, sd, cfg["optim"], cfg["model"], batch)
    _check_train(d, loss, y, grads, after, check_y=False)


@pytest.mark.slow
def test_metaformer_full_width_train_step():
    from tests.model_shapes import empty_state_dict
    d = load("metaformer_full_r1")
    cfg = config(d)
    sd = empty_state_dict("Metaformer")
    # same sorted-key RandomState filler (synthetic.fill_params_randomstate) the golden
    # generator applied to the reference
    rs = np.random.RandomState(2)
    for k in sorted(sd):
        arr = rs.standard_normal(tuple(sd[k].shape)).astype(np.float32) * 0.08
        if "layer_norm.weight" in k or k.endswith("norm.weight"):
            arr = arr + 1.0
        sd[k] = torch.from_numpy(arr)
    batch = batch_from(d)
    loss, y, grads, after = O.run_train_step(O.metaformer_training_loss, sd, cfg["optim"], cfg["model"], batch)
    with torch.no_grad():
        inp = list(batch[:-1])
        ms = inp[2][0]
        inp[2] = (ms * (ms != -100).int(), inp[2][1])
        assert rel_err(O.metaformer_forward(sd, cfg["model"], inp), d["y"]) < TOL
    _check_train(d, loss, y, grads, after, check_y=False)


def test_lstm_with_sample_teacher_forced():
    d = load("lstm_with_sample_tf")
    cfg = config(d)
    sd = prefixed(d, "param/")
    batch = batch_from(d)
    with torch.no_grad():
        y, _ = O.lstm_with_sample_forward(sd, cfg["model"], batch[:-1])
        assert rel_err(y, d["y"]) < TOL
    loss, y, grads, after = O.run_train_step(O.lstm_with_sample_training_loss, sd, cfg["optim"], cfg["model"], batch)
    _check_train(d, loss, y, grads, after, check_y=False)


def test_lstm_with_sample_scheduled_sampling():
    d = load("lstm_with_sample_ss")
    cfg = config(d)
    sd = prefixed(d, "param/")
    batch = batch_from(d)
    mask = torch.from_numpy(d["sampling_mask"])
    loss, y, grads, after = O.run_train_step(O.lstm_with_sample_training_loss, sd, cfg["optim"], cfg["model"],
                                             batch, sampling_mask=mask)
    _check_train(d, loss, y, grads, after, check_y=False)


def test_simple_lstm_train_step():
    d = load("simple_lstm_small")
    cfg = config(d)
    sd = prefixed(d, "param/")
    a, m, t = (torch.from_numpy(d[k]) for k in ("in/audio", "in/motion", "in/target"))
    with torch.no_grad():
        assert rel_err(O.simple_lstm_forward(sd, cfg["model"], a, m), d["y"]) < TOL
    loss, y, grads, after = O.run_train_step(O.simple_lstm_training_loss, sd, cfg["optim"], cfg["model"], a, m, t)
    _check_train(d, loss, y, grads, after, check_y=False)


@pytest.mark.parametrize("reverse", [False, True])
def test_aten_lstm_timing_path_equals_restatement(reverse):
    """The fused ATen LSTM (what bench.py's CPU baseline times) == the oracle's per-step loop."""
    g = torch.Generator().manual_seed(3)
    B, T, In, H = 3, 17, 12, 8
    x = torch.randn(B, T, In, generator=g, requires_grad=True)
    ws = [torch.randn(4 * H, In, generator=g) * 0.3, torch.randn(4 * H, H, generator=g) * 0.3,
          torch.randn(4 * H, generator=g) * 0.1, torch.randn(4 * H, generator=g) * 0.1]
    h0, c0 = torch.randn(B, H, generator=g), torch.randn(B, H, generator=g)
    outs = []
    for aten in (False, True):
        O.ATEN_LSTM = aten
        try:
            xx = x.detach().clone().requires_grad_(True)
            y, hT, cT = O.lstm_layer(xx, *ws, h0, c0, reverse=reverse)
            (y.square().sum() + hT.sum() + cT.sum()).backward()
            outs.append((y.detach(), hT.detach(), cT.detach(), xx.grad))
        finally:
            O.ATEN_LSTM = False
    for a, b in zip(*outs):
        assert rel_err(a, b) < 1e-5


@pytest.mark.parametrize("mode", ["full", "tf", "ss"])
def test_metaformer_generation(mode):
    """Metaformer.prediction (lstmformer.py:426-547) at ratio 2 with ragged -100 padding:
    full generation, teacher forcing and the recorded scheduled-sampling mask."""
    d = load("metaformer_gen_r2_pad")
    cfg = config(d)
    sd = prefixed(d, "param/")
    batch = batch_from(d)
    T = batch[1][0].shape[1]
    mask = {"full": torch.ones(T, dtype=torch.bool), "tf": torch.zeros(T, dtype=torch.bool),
            "ss": torch.from_numpy(d["sampling_mask"])}[mode]
    with torch.no_grad():
        pred = O.metaformer_prediction(sd, cfg["model"], batch, mask)
    assert rel_err(pred, d[f"pred/{mode}"]) < TOL


def test_metaformer_q9_broadcast_losses():
    """SURVEY Q9 (lstmformer.py:434-435): prediction's target broadcasts to [T,B,T,F]; the
    reference's genrt_loss (generation_step) and scheduled-sampling training_step loss + grads +
    AdamW step are taken over it (ragged padding, delta_order 1, delta_loss_scale 2)."""
    d = load("metaformer_q9_r2_pad")
    cfg = config(d)
    sd = prefixed(d, "param/")
    batch = batch_from(d)
    T = batch[1][0].shape[1]
    with torch.no_grad():
        pred = O.metaformer_prediction(sd, cfg["model"], batch, torch.zeros(T, dtype=torch.bool))
        assert rel_err(pred, d["gen/pred"]) < TOL
        t4 = O.metaformer_prediction_target(batch)
        assert t4.shape == d["gen/target4"].shape and torch.equal(t4.float(), torch.from_numpy(d["gen/target4"]))
        g = O.metaformer_genrt_loss(sd, cfg["model"], batch)
        assert abs(g.item() - float(d["genrt_loss"])) / float(d["genrt_loss"]) < TOL
    mask = torch.from_numpy(d["sampling_mask"])
    loss, y, grads, after = O.run_train_step(O.metaformer_ss_training_loss, sd, cfg["optim"], cfg["model"],
                                             batch, sampling_mask=mask)
    _check_train(d, loss, y, grads, after, check_y=False)


def test_feature_log_power_and_deltas_golden():
    """compute_log_power (audio.py:43-56) and compute_delta (audio.py:58-67) as the reference
    itself computed them (tests/golden/features.npz): bit-exact."""
    d = load("features")
    lp = O.compute_log_power(torch.from_numpy(d["wave"]), 400, 160)
    assert torch.equal(lp, torch.from_numpy(d["log_power"]))
    x = torch.from_numpy(d["delta_in"])
    for k in range(3):
        assert torch.equal(O.compute_delta(x, k), torch.from_numpy(d[f"delta{k}"])), k


def test_mel_filterbank_restatement_properties():
    """The torchaudio HTK filterbank restatement (parity unpinned: torchaudio is absent):
    triangles of peak <= 1 with successive, overlapping supports covering 0..sr/2."""
    fb = O.melscale_fbanks_htk(201, 0.0, 8000.0, 26, 16000)
    assert fb.shape == (201, 26) and fb.dtype == torch.float32
    assert float(fb.min()) == 0.0 and float(fb.max()) <= 1.0
    peaks = fb.argmax(0)
    assert bool((peaks[1:] > peaks[:-1]).all())
    assert bool((fb.sum(1)[1:-1] > 0).all())


def test_feature_constants_match_restatement():
    """The product's constant tables (features.py, built on the host) against the oracle:
    the filterbank equals the restatement and the DFT basis reproduces |torch.stft|^2."""
    from multimodalreactiongeneration_amd import features as FT
    assert torch.equal(FT.melscale_fbanks(201, 0.0, 8000.0, 40, 16000), O.melscale_fbanks_htk(201, 0.0, 8000.0, 40, 16000))
    g = torch.Generator().manual_seed(3)
    x = torch.randn(400 + 160 * 4, generator=g, dtype=torch.float64)
    basis = FT.dft_basis(400).double()
    frames = x.unfold(0, 400, 160)
    spec = frames @ basis.t()
    p = spec[:, :201] ** 2 + spec[:, 201:] ** 2
    ref = torch.stft(x, 400, 160, 400, torch.hann_window(400, dtype=torch.float64), center=False,
                     return_complex=True).abs().pow(2).t()
    assert rel_err(p, ref) < 1e-6


@pytest.mark.parametrize("rev,state", [(False, False), (True, True)])
def test_gru_restatement_matches_nn_gru(rev, state):
    """oracle.gru_layer vs torch.nn.GRU itself (the op GRUMixer wraps, mixer_block.py:193-201)."""
    torch.manual_seed(5)
    gru = torch.nn.GRU(7, 12, batch_first=True, bidirectional=rev)
    x = torch.randn(3, 9, 7)
    h0 = torch.randn(2 if rev else 1, 3, 12) if state else None
    y, hn = gru(x, h0)
    d = 1 if rev else 0
    sfx = "_reverse" if rev else ""
    w = [getattr(gru, f"{n}_l0{sfx}") for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    yo, ho = O.gru_layer(x, *w, None if h0 is None else h0[d], reverse=rev)
    assert rel_err(yo, y[..., d * 12:(d + 1) * 12]) < 1e-5
    assert rel_err(ho, hn[d]) < 1e-5


def test_fp32_oracle_vs_b64_float64_fixture():
    """The float64 B=64 T=300 fixture the GPU test of the benchmarked schedule is checked against
    (tests/golden/make_b64_fixture.py) vs this fp32 oracle on the same inputs: the loss and every
    sampled gradient within the GPU test's tolerances (1e-4; 2e-3 for the ReLU FeedForward input
    layers, whose kink flips under fp32 rounding: measured 3.8e-4 here)."""
    from multimodalreactiongeneration_amd import configs as C
    from multimodalreactiongeneration_amd.model import Metaformer
    from multimodalreactiongeneration_amd.synthetic import make_batch
    d = load("metaformer_b64_f64")
    mc, oc, me = C.lstmformer_config(ratio=1)
    torch.manual_seed(0)
    sd = {k: v.detach().clone() for k, v in Metaformer(mc, oc, me).state_dict().items()}
    assert abs(sum(v.double().sum().item() for v in sd.values()) - float(d["param_sum"])) < 1e-6
    prev = O.ATEN_LSTM
    O.ATEN_LSTM = True
    try:
        loss, _, grads, _ = O.run_train_step(O.metaformer_training_loss, sd, oc, mc,
                                             make_batch(B=64, T=300, ratio=1, seed=1234))
    finally:
        O.ATEN_LSTM = prev
    assert abs(loss.item() - float(d["loss"])) / abs(float(d["loss"])) < TOL
    for k, g in grads.items():
        tol = 2e-3 if ".feedforward.feed_forward.module.input." in k else TOL
        gmax = d[f"stat/{k}"][0]
        e = (g.reshape(-1).double()[torch.from_numpy(d[f"idx/{k}"])] - torch.from_numpy(d[f"g/{k}"])).abs().max()
        assert e.item() / max(gmax, 1e-30) < tol, k


def _sampled_grads_within(d, loss, grads, tol_of=lambda k: TOL):
    assert abs(loss.item() - float(d["loss"])) / abs(float(d["loss"])) < TOL
    for k, g in grads.items():
        gmax = d[f"stat/{k}"][0]
        e = (g.reshape(-1).double()[torch.from_numpy(d[f"idx/{k}"])] - torch.from_numpy(d[f"g/{k}"])).abs().max()
        assert e.item() / max(gmax, 1e-30) < tol_of(k), k


def test_fp32_oracle_vs_c3_b64_float64_fixture():
    """The float64 fixture of bench.py's C3 step (LSTMwithSample scheduled sampling, B=64, T=300, lead 12,
    tests/golden/make_b64_fixture.py) vs this fp32 oracle: the fixture is the oracle's own answer in
    float64, so the fp32 restatement sits within the GPU test's 1e-4 of it (lstm_with_sample.py:379-433)."""
    from multimodalreactiongeneration_amd import configs as C
    from multimodalreactiongeneration_amd.model import LSTMwithSample
    from multimodalreactiongeneration_amd.synthetic import make_batch
    d = load("lstm_with_sample_ss_b64_f64")
    mc, oc, me = C.lstm_with_sampling_config(use_scheduled_sampling=True)
    torch.manual_seed(0)
    sd = {k: v.detach().clone() for k, v in LSTMwithSample(mc, oc, me).state_dict().items()}
    assert abs(sum(v.double().sum().item() for v in sd.values()) - float(d["param_sum"])) < 1e-6
    loss, y, grads, _ = O.run_train_step(O.lstm_with_sample_training_loss, sd, oc, mc,
                                         make_batch(B=64, T=300, lead=12, seed=1234),
                                         sampling_mask=torch.from_numpy(d["sampling_mask"]))
    assert rel_err(y, d["y"]) < TOL
    _sampled_grads_within(d, loss, grads)


def test_fp32_oracle_vs_generation_b64_float64_fixture():
    """Metaformer.prediction at B=64 on 40 frames (full and scheduled-sampling masks) in fp32 vs the
    float64 fixture the GPU generation test uses (lstmformer.py:426-547)."""
    from multimodalreactiongeneration_amd import configs as C
    from multimodalreactiongeneration_amd.model import Metaformer
    from multimodalreactiongeneration_amd.synthetic import make_batch
    d = load("metaformer_gen_b64_f64")
    mc, oc, me = C.lstmformer_config(ratio=1)
    torch.manual_seed(0)
    sd = {k: v.detach().clone() for k, v in Metaformer(mc, oc, me).state_dict().items()}
    batch = make_batch(B=64, T=40, lead=12, seed=1234)
    with torch.no_grad():
        for mode in ("full", "ss"):
            pred = O.metaformer_prediction(sd, mc, batch, torch.from_numpy(d[f"mask/{mode}"]))
            assert rel_err(pred, d[f"pred/{mode}"]) < TOL, mode


@pytest.mark.slow
def test_fp32_oracle_vs_c2_b64_float64_fixture():
    """simple_lstm fp32 at B=64, T=300 (bench.py step_c2) vs its float64 fixture (simple_lstm.py:181-255)."""
    from multimodalreactiongeneration_amd import configs as C
    from multimodalreactiongeneration_amd.model import SimpleLSTM
    from multimodalreactiongeneration_amd.synthetic import make_simple_batch
    d = load("simple_lstm_b64_f64")
    cfg, oc, me = C.simple_lstm_config()
    torch.manual_seed(0)
    sd = {k: v.detach().clone() for k, v in SimpleLSTM(cfg, oc, me).state_dict().items()}
    prev = O.ATEN_LSTM
    O.ATEN_LSTM = True
    try:
        loss, y, grads, _ = O.run_train_step(O.simple_lstm_training_loss, sd, oc, cfg, *make_simple_batch(B=64, T=300))
    finally:
        O.ATEN_LSTM = prev
    assert rel_err(y, d["y"]) < TOL
    _sampled_grads_within(d, loss, grads)


@pytest.mark.parametrize("reverse", [False, True])
def test_aten_gru_timing_path_equals_restatement(reverse):
    """The fused ATen GRU (what bench.py's GRU-config CPU baseline times) == the oracle's per-step loop."""
    g = torch.Generator().manual_seed(4)
    B, T, In, H = 3, 17, 12, 8
    x = torch.randn(B, T, In, generator=g)
    w = [torch.randn(3 * H, In, generator=g), torch.randn(3 * H, H, generator=g),
         torch.randn(3 * H, generator=g), torch.randn(3 * H, generator=g)]
    h0 = torch.randn(B, H, generator=g)
    y0, h0_ = O.gru_layer(x, *w, h0, reverse=reverse)
    prev = O.ATEN_LSTM
    O.ATEN_LSTM = True
    try:
        y1, h1 = O.gru_layer(x, *w, h0, reverse=reverse)
    finally:
        O.ATEN_LSTM = prev
    assert rel_err(y1, y0) < 1e-5 and rel_err(h1, h0_) < 1e-5


def test_relu_mask_injection_is_the_identity_at_the_own_kinks():
    """oracle.RELU_MASKS (the GPU B=64 checks evaluate the float64 oracle at the GPU forward's ReLU
    sides): injecting the masks the oracle's own forward decides gives bitwise its own loss and
    gradients; flipping the sides of one sample's rows changes the result (the masks are really used); a mask of
    the wrong shape is refused."""
    d = load("metaformer_small_r2_pad")
    cfg = config(d)
    sd = prefixed(d, "param/")
    batch = batch_from(d)
    seen = {}
    real = O.relu

    def record(x, prefix):
        seen[prefix] = x > 0
        return real(x, prefix)
    O.relu = record
    try:
        base = O.run_train_step(O.metaformer_training_loss, sd, cfg["optim"], cfg["model"], batch)
    finally:
        O.relu = real
    assert sorted(seen) == sorted({k[:-len("weight")] for k in sd if k.endswith("input.weight")})
    try:
        O.RELU_MASKS = seen
        inj = O.run_train_step(O.metaformer_training_loss, sd, cfg["optim"], cfg["model"], batch)
        assert torch.equal(inj[0], base[0])
        for k in base[2]:
            assert torch.equal(inj[2][k], base[2][k]), k
        key = sorted(seen)[-1]
        flipped = seen[key].clone()
        flipped[0] = ~flipped[0]
        O.RELU_MASKS = dict(seen, **{key: flipped})
        moved = O.run_train_step(O.metaformer_training_loss, sd, cfg["optim"], cfg["model"], batch)
        assert not torch.equal(moved[2][key + "weight"], base[2][key + "weight"])
        O.RELU_MASKS = {key: flipped[..., :-1]}
        with pytest.raises(ValueError):
            O.run_train_step(O.metaformer_training_loss, sd, cfg["optim"], cfg["model"], batch)
    finally:
        O.RELU_MASKS = None


def test_relu_mask_bound_rejects_a_far_flip_and_accepts_a_kink_flip():
    """The bound the GPU checks put on injected ReLU masks (golden_util.relu_flips_ok over
    oracle.RELU_STATS, band 1e-5 of the layer's rms, at most 32 flips) can fail: in float64 on the small
    config, the oracle's own masks pass with 0 flips; one entry flipped at |z| > 1e-2 rms is rejected,
    its layer's record holding exactly that flip; one entry flipped at |z| <= band rms (made by moving
    that layer's input bias so the pre-activation lands on the kink) is accepted and counted as 1."""
    from tests.golden_util import relu_flips_ok, relu_flip_totals
    band = 1e-5
    d = load("metaformer_small_r2_pad")
    cfg = config(d)
    sd = {k: v.double() for k, v in prefixed(d, "param/").items()}
    batch = [(x.double(), n) for x, n in batch_from(d)]
    real = O.relu

    def own(sd_):
        """{prefix: pre-activation} of the oracle's own forward."""
        seen = {}

        def record(x, prefix):
            seen[prefix] = x.detach().clone()
            return real(x, prefix)
        O.relu = record
        try:
            O.metaformer_training_loss(sd_, cfg["model"], batch)
        finally:
            O.relu = real
        return seen

    def stats_at(sd_, masks):
        O.RELU_MASKS, O.RELU_STATS, O.RELU_BAND = masks, {}, band
        try:
            O.metaformer_training_loss(sd_, cfg["model"], batch)
            return O.RELU_STATS
        finally:
            O.RELU_MASKS, O.RELU_STATS, O.RELU_BAND = None, None, 1e-5

    z = own(sd)
    masks = {k: v > 0 for k, v in z.items()}
    key = "metaformer.metaformer_blocks.0.feedforward.feed_forward.module.input."
    assert key in z and len(z) > 1
    st = stats_at(sd, masks)
    assert sorted(st) == sorted(z) and all(s["n"] == z[k].numel() for k, s in st.items())
    assert relu_flips_ok(st, band) and relu_flip_totals(st)[0] == 0

    # a flip far from the kink
    rms = z[key].pow(2).mean().sqrt().item()
    at = int(z[key].abs().argmax())
    zf = abs(z[key].reshape(-1)[at].item())
    assert zf > 1e-2 * rms
    far = {k: v.clone() for k, v in masks.items()}
    far[key].view(-1)[at] ^= True
    st = stats_at(sd, far)
    assert st[key]["flips"] == 1 and st[key]["max_flip"] == zf and abs(st[key]["rms"] - rms) <= 1e-12 * rms
    assert not relu_flips_ok(st, band)
    assert relu_flip_totals(st)[1] >= zf / rms and relu_flip_totals(st)[0] >= 1

    # a flip on the kink: move bias[j] so that entry (i, j) of this layer's pre-activation is ~0
    j = at % z[key].shape[-1]
    sd2 = dict(sd)
    sd2[key + "bias"] = sd[key + "bias"].clone()
    sd2[key + "bias"][j] -= z[key].reshape(-1)[at]
    z2 = own(sd2)
    rms2 = z2[key].pow(2).mean().sqrt().item()
    assert abs(z2[key].reshape(-1)[at].item()) <= band * rms2
    near = {k: v > 0 for k, v in z2.items()}
    near[key].view(-1)[at] ^= True
    st = stats_at(sd2, near)
    assert relu_flips_ok(st, band)
    flips, worst, where, n_near = relu_flip_totals(st)
    assert flips == 1 and st[key]["flips"] == 1 and where == key and worst <= band and n_near >= 1
    assert not relu_flips_ok(st, band, max_flips=0)
    assert not relu_flips_ok({}, band)   # nothing recorded: nothing checked

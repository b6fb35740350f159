"""bin/ac_ppo_carla --use_positional_encoding 1 against the scripted leaderboard gyms of
test_gpu_carla_trainer_app.py (2 envs, T = 4, 1 epoch of 2 minibatches): one iteration writes a model whose
cnn.0.weight is [8, 17, 5, 5] and a config.json that carries the switch; a second run resumes from them
without the flag (the switch comes from config.json) and trains on."""
import json
import os
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
ppo_amd = pytest.importorskip("ppo_amd")

import test_gpu_carla_trainer_app as TA  # noqa: E402


def test_trainer_with_positional_encoding_checkpoints_and_resumes():
    assert os.path.exists(TA.APP), "bin/ac_ppo_carla not built (run __graft_entry__.build())"
    L = ppo_amd.carla_layout2(positional_encoding=True)
    with tempfile.TemporaryDirectory() as d:
        comm, logdir = os.path.join(d, "team_code"), os.path.join(d, "logs")
        out = TA._run(comm, logdir, "pos", 8, ("--use_positional_encoding", "1"))
        assert "SPS:" in out, out
        folder = os.path.join(logdir, "pos")
        model = os.path.join(folder, "model_latest_000000000.pth")
        assert TA._latest(folder) == (["model_latest_000000000.pth"], ["optimizer_latest_000000000.pth"])
        sd = dict(torch.jit.load(model).named_parameters())
        assert tuple(sd["cnn.0.weight"].shape) == (8, 17, 5, 5)
        # fresh convolutions as the reference's _weights_init draws them (carla_model.h:555-560):
        # xavier_uniform_ with gain sqrt(2), fan_in (15 + 2) * 25, fan_out 8 * 25, bias 0.1. Two Adam steps of
        # at most 3e-4 each have moved every entry by less than 1e-3. The largest of 3 400 uniform draws
        # misses 0.9 x the bound with probability 0.9 ** 3400.
        bound = np.sqrt(2.0) * np.sqrt(6.0 / ((17 + 8) * 25))  # 0.1386
        wmax = float(sd["cnn.0.weight"].detach().abs().max())
        assert 0.9 * bound < wmax < bound + 1e-3, (wmax, bound)
        for i in range(0, 12, 2):  # roach: Conv2d, ReLU
            assert float((sd["cnn.%d.bias" % i].detach() - 0.1).abs().max()) < 1e-3, i
        p0 = ppo_amd.load_carla_pth2(L, model)
        assert np.isfinite(p0).all() and p0.size == ppo_amd.carla_layout2().P + 400
        with open(os.path.join(folder, "config.json")) as f:
            assert json.load(f)["use_positional_encoding"] is True
        m, v, step, _, _ = ppo_amd.load_carla_adam_pth2(L, os.path.join(folder, "optimizer_latest_000000000.pth"))
        assert step == 2
        w0 = slice(L.conv_w[0], L.conv_w[0] + 8 * 17 * 25)
        assert np.abs(m[w0].reshape(8, 17, 25)[:, 15:]).max() > 0  # the positional weights are trained

        # resume: iteration 1 only; config.json brings the switch back
        out = TA._run(comm, logdir, "pos", 16, ("--load_file", model))
        assert "Start training from step: 1" in out and out.count("SPS:") == 1, out
        assert TA._latest(folder) == (["model_latest_000000001.pth"], ["optimizer_latest_000000001.pth"])
        p1 = ppo_amd.load_carla_pth2(L, os.path.join(folder, "model_latest_000000001.pth"))
        assert np.isfinite(p1).all() and not np.array_equal(p1, p0)
        _, _, step, _, _ = ppo_amd.load_carla_adam_pth2(L, os.path.join(folder, "optimizer_latest_000000001.pth"))
        assert step == 4

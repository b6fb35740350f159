"""CPU-side checks of the CaRL act lanes' C-ABI (include/ppo_carla.h, "act lanes") and of the trainer's
--collect_mode flag: the entry points are exported and bound, NULL arguments are refused with a message
before any HIP call (there is no GPU here, so a HIP call would fail differently), and an unknown mode is
a parse error.

A lane exists only beside a rollout object, and a rollout object only beside an agent on a device. The
refusals that need a lane handle — a step or env outside the storage, a 65th lane — are therefore the
two tests marked gpu at the end: they hand every lane call HOST addresses that no HIP call could take,
so a refusal with the argument's message is a refusal before any HIP call."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "ppo.cpp_amd", "lib", "libppo_hip.so")
APP = os.path.join(ROOT, "ppo.cpp_amd", "bin", "ac_ppo_carla")

SYMS = ["ppo_carla_lane_create", "ppo_carla_lane_destroy", "ppo_carla_lane_act", "ppo_carla_lane_reward",
        "ppo_carla_lane_sync", "ppo_carla_debug_lane_in"]


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(LIB), "libppo_hip.so not built (run __graft_entry__.build())"
    import ppo_amd
    return ppo_amd.lib()


def _err(lib):
    return lib.ppo_last_error().decode()


def test_lane_symbols_are_exported_and_bound(lib):
    import ppo_amd
    raw = C.CDLL(LIB)
    assert [s for s in SYMS if not hasattr(raw, s)] == []
    assert set(SYMS) <= {n for n, _, _ in ppo_amd.SYMBOLS}
    assert hasattr(ppo_amd, "CarlaLane") and hasattr(ppo_amd.CarlaRollout, "lane")


def test_lane_calls_refuse_null_arguments(lib):
    out = C.c_void_p()
    x = C.cast(C.create_string_buffer(64), C.c_void_p)
    assert lib.ppo_carla_lane_create(None, C.byref(out)) != 0
    assert "ppo_carla_lane_create: null argument" in _err(lib) and not out.value
    # the rollout object is not dereferenced before the NULL checks: any non-NULL address stands in for one
    assert lib.ppo_carla_lane_create(x, None) != 0 and "ppo_carla_lane_create: null argument" in _err(lib)
    assert lib.ppo_carla_lane_act(None, 0, 0, x, x, x, 0.0, x) != 0 and "ppo_carla_lane_act: null argument" in _err(lib)
    assert lib.ppo_carla_lane_reward(None, 0, 0, 1.0) != 0 and "ppo_carla_lane_reward: null argument" in _err(lib)
    assert lib.ppo_carla_lane_sync(None) != 0 and "ppo_carla_lane_sync: null argument" in _err(lib)
    assert lib.ppo_carla_lane_destroy(None) == 0


def test_debug_lane_in_refuses_bad_arguments(lib):
    x = C.cast(C.create_string_buffer(64), C.c_void_p)
    assert lib.ppo_carla_debug_lane_in(-1, 0, x, x, 0.0, 0.0, x, x, x, x, None) != 0
    assert "ppo_carla_debug_lane_in" in _err(lib)
    assert lib.ppo_carla_debug_lane_in(2, 0, None, None, 0.0, 0.0, x, None, x, x, None) != 0
    assert "ppo_carla_debug_lane_in: null argument" in _err(lib)
    assert lib.ppo_carla_debug_lane_in(2, 1, x, x, 0.0, 0.0, x, None, x, x, None) != 0
    assert "ppo_carla_debug_lane_in: null argument" in _err(lib)


def test_trainer_refuses_an_unknown_collect_mode(tmp_path):
    assert os.path.exists(APP), "bin/ac_ppo_carla not built (run __graft_entry__.build())"
    r = subprocess.run([APP, "--team_code_folder", str(tmp_path), "--collect_mode", "bogus"], capture_output=True,
                       text=True, timeout=60, cwd=tmp_path)
    assert r.returncode == 1, (r.returncode, r.stdout[-500:], r.stderr[-500:])
    assert "collect_mode" in r.stderr and "bogus" in r.stderr
    h = subprocess.run([APP, "--help"], capture_output=True, text=True, timeout=60, cwd=tmp_path)
    assert h.returncode == 0 and "collect_mode" in h.stdout and "lockstep" in h.stdout and "threads" in h.stdout


# ---- with a lane handle: needs a rollout object, hence a device ------------------------------------
@pytest.fixture()
def rollout():
    import ppo_amd
    ppo_amd.set_device(0)
    agent = ppo_amd.CarlaAgent(max_batch=6, seed=5)
    ro = ppo_amd.CarlaRollout(agent, num_steps=2, num_envs=3, update_epochs=1, num_minibatches=3)
    yield ro
    ro.close()
    agent.close()


@pytest.mark.gpu
def test_lane_refuses_a_step_or_env_outside_the_storage(lib, rollout):
    lane = rollout.lane()
    L = rollout.agent.layout2
    bev = np.zeros(L.C * L.IH * L.IW, np.uint8)
    f = np.zeros(16, np.float32)
    act = np.full(L.A, 7.0, np.float32)
    for step, env, word in [(-1, 0, "step"), (2, 0, "step"), (0, -1, "env"), (0, 3, "env"), (1 << 30, 0, "step")]:
        rc = lib.ppo_carla_lane_act(lane._h, step, env, bev.ctypes.data, f.ctypes.data, f.ctypes.data, 0.0,
                                    act.ctypes.data)
        assert rc != 0 and f"ppo_carla_lane_act: {word} out of range" in _err(lib), (step, env, _err(lib))
        rc = lib.ppo_carla_lane_reward(lane._h, step, env, 1.0)
        assert rc != 0 and f"ppo_carla_lane_reward: {word} out of range" in _err(lib), (step, env, _err(lib))
    assert (act == 7.0).all()
    # NULL arrays beside a live handle
    assert lib.ppo_carla_lane_act(lane._h, 0, 0, None, f.ctypes.data, f.ctypes.data, 0.0, act.ctypes.data) != 0
    assert "ppo_carla_lane_act: null argument" in _err(lib)
    assert lib.ppo_carla_lane_act(lane._h, 0, 0, bev.ctypes.data, f.ctypes.data, None, 0.0, act.ctypes.data) != 0
    assert "ppo_carla_lane_act: null argument" in _err(lib)
    assert lib.ppo_carla_lane_act(lane._h, 0, 0, bev.ctypes.data, f.ctypes.data, f.ctypes.data, 0.0, None) != 0
    assert "ppo_carla_lane_act: null argument" in _err(lib)
    # the storage saw none of it
    for name in ("dones", "rewards", "values", "meas"):
        assert not rollout.buffer(name).numpy().any(), name


@pytest.mark.gpu
def test_a_rollout_object_has_at_most_64_lanes(lib, rollout):
    lanes = [rollout.lane() for _ in range(64)]
    extra = C.c_void_p()
    assert lib.ppo_carla_lane_create(rollout._h, C.byref(extra)) != 0
    assert "at most 64 lanes" in _err(lib) and not extra.value
    lanes[10].close()  # a freed slot serves again
    again = rollout.lane()
    assert lib.ppo_carla_lane_create(rollout._h, C.byref(extra)) != 0 and not extra.value
    again.sync()

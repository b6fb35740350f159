"""CPU-side checks of the CaRL rollout object's C-ABI (include/ppo_carla.h, "rollout storage, GAE and
the epoch loop"): the entry points are exported and bound, and every argument error is refused with a
message before any HIP call (there is no GPU here, so a HIP call would fail differently)."""
import ctypes as C
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "ppo.cpp_amd", "lib", "libppo_hip.so")

SYMS = ["ppo_carla_rollout_create", "ppo_carla_rollout_destroy", "ppo_carla_rollout_act", "ppo_carla_rollout_reward",
        "ppo_carla_rollout_gae", "ppo_carla_rollout_train", "ppo_carla_rollout_buffer", "ppo_carla_rollout_last_perms",
        "ppo_carla_rollout_iteration", "ppo_carla_rollout_set_iteration", "ppo_carla_debug_gather",
        "ppo_carla_debug_gather_f32"]


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(LIB), "libppo_hip.so not built (run __graft_entry__.build())"
    import ppo_amd
    return ppo_amd.lib()


def _err(lib):
    return lib.ppo_last_error().decode()


def test_rollout_symbols_are_exported_and_bound(lib):
    import ppo_amd
    raw = C.CDLL(LIB)
    assert [s for s in SYMS if not hasattr(raw, s)] == []
    assert set(SYMS) <= {n for n, _, _ in ppo_amd.SYMBOLS}


def test_rollout_create_refuses_null_arguments(lib):
    import ppo_amd
    out = C.c_void_p()
    cfg = ppo_amd.CarlaRolloutConfig(6, 4, 2, 3, 0.99, 0.95, 1, 0)
    assert lib.ppo_carla_rollout_create(None, C.byref(cfg), C.byref(out)) != 0
    assert "ppo_carla_rollout_create" in _err(lib) and not out.value
    # the agent is not dereferenced before the NULL checks: any non-NULL address stands in for one
    fake = C.create_string_buffer(64)
    assert lib.ppo_carla_rollout_create(C.cast(fake, C.c_void_p), None, C.byref(out)) != 0
    assert "ppo_carla_rollout_create" in _err(lib) and not out.value


def test_rollout_calls_refuse_a_null_handle(lib):
    import ppo_amd
    tc = ppo_amd.CarlaTrainConfig(0.2, 0.0, 0.5, 0.5, 1e-5, 1, 1)
    x = C.cast(C.create_string_buffer(64), C.c_void_p)
    assert lib.ppo_carla_rollout_act(None, 0, 0, 1, x, x, x, x, None, None) != 0 and "rollout_act" in _err(lib)
    assert lib.ppo_carla_rollout_reward(None, 0, 0, 1, x, None) != 0 and "rollout_reward" in _err(lib)
    assert lib.ppo_carla_rollout_gae(None, x, x, x, x, 1, None) != 0 and "rollout_gae" in _err(lib)
    assert lib.ppo_carla_rollout_train(None, C.byref(tc), 1e-3, 1, None, None, None) != 0
    assert "rollout_train" in _err(lib)
    assert lib.ppo_carla_rollout_iteration(None) == -1
    assert lib.ppo_carla_rollout_destroy(None) == 0


def test_debug_gather_refuses_bad_arguments(lib):
    x = C.cast(C.create_string_buffer(64), C.c_void_p)
    for n, rb, src, idx, dst in [(-1, 16, x, x, x), (1, 0, x, x, x), (1, -16, x, x, x), (1, 16, None, x, x),
                                 (1, 16, x, None, x), (1, 16, x, x, None)]:
        assert lib.ppo_carla_debug_gather(n, rb, src, idx, dst, None) != 0, (n, rb)
        assert "ppo_carla_debug_gather" in _err(lib)
    ptrs = (C.c_void_p * 1)(x.value)
    w = (C.c_int * 1)(3)
    assert lib.ppo_carla_debug_gather_f32(-1, 1, ptrs, w, x, ptrs, None) != 0
    assert lib.ppo_carla_debug_gather_f32(1, 9, ptrs, w, x, ptrs, None) != 0
    assert lib.ppo_carla_debug_gather_f32(1, 1, None, w, x, ptrs, None) != 0
    assert "ppo_carla_debug_gather_f32" in _err(lib)

"""CPU-side checks of the evaluation call's C-ABI (include/ppo_synth_env.h, ppo_evaluate_synth) and of the
fourth sample type: the entry points are exported and bound, the ctypes restatement of ppo_eval_config
has the header's size and field offsets, and argument errors are refused with a message before any HIP
call (there is no GPU here, so a HIP call would fail differently)."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "ppo.cpp_amd", "lib", "libppo_hip.so")

SYMS = ["ppo_evaluate_synth", "ppo_eval_info"]
FIELDS = ["sample_type", "eval_seed", "num_eval_envs", "num_eval_runs", "step0", "chunk_steps", "mode"]


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(LIB), "libppo_hip.so not built (run __graft_entry__.build())"
    import ppo_amd
    return ppo_amd.lib()


def test_eval_symbols_are_exported_and_bound(lib):
    import ppo_amd
    raw = C.CDLL(LIB)
    assert [s for s in SYMS if not hasattr(raw, s)] == []
    assert set(SYMS) <= {n for n, _, _ in ppo_amd.SYMBOLS}


def test_roach_constant_matches_the_header(tmp_path):
    import ppo_amd
    assert ppo_amd.PPO_ROACH == 3
    assert (ppo_amd.PPO_SAMPLE, ppo_amd.PPO_MEAN, ppo_amd.PPO_GIVEN) == (0, 1, 2)
    src = '#include <stdio.h>\n#include "ppo_hip.h"\nint main(void) { printf("%d %d %d %d", PPO_SAMPLE, PPO_MEAN, PPO_GIVEN, PPO_ROACH); return 0; }\n'
    (tmp_path / "e.c").write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "e.c"), "-o", str(tmp_path / "e")])
    assert subprocess.check_output([str(tmp_path / "e")]).decode().split() == ["0", "1", "2", "3"]


def test_eval_config_struct_matches_the_header(tmp_path):
    """sizeof(ppo_eval_config) and every field's offset and size, compiled from the header, against
    the ctypes structure the Python binding passes."""
    import ppo_amd
    assert [f for f, _ in ppo_amd.EvalConfig._fields_] == FIELDS
    prints = "".join(f'  printf(" %zu:%zu", offsetof(ppo_eval_config, {f}), sizeof(((ppo_eval_config*)0)->{f}));\n'
                     for f in FIELDS)
    src = ('#include <stddef.h>\n#include <stdio.h>\n#include "ppo_synth_env.h"\nint main(void) {\n'
           '  printf("%zu", sizeof(ppo_eval_config));\n' + prints + "  return 0;\n}\n")
    (tmp_path / "s.c").write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "s.c"), "-o", str(tmp_path / "s")])
    out = subprocess.check_output([str(tmp_path / "s")]).decode().split()
    assert int(out[0]) == C.sizeof(ppo_amd.EvalConfig)
    for f, tok in zip(FIELDS, out[1:]):
        d = getattr(ppo_amd.EvalConfig, f)
        assert tok == f"{d.offset}:{d.size}", f


def test_evaluate_refuses_null_arguments(lib):
    """NULL checks come before anything is dereferenced: any non-NULL address stands in for a handle."""
    import ppo_amd
    x = C.cast(C.create_string_buffer(256), C.c_void_p)
    cfg = ppo_amd.EvalConfig(ppo_amd.PPO_MEAN, 2, 1, 2, 0, 0, 0)
    n, steps = C.c_int(-7), C.c_long(-7)
    assert lib.ppo_evaluate_synth(x, x, None, x, x, 2, C.byref(n), C.byref(steps)) != 0  # NULL config
    assert "ppo_evaluate_synth" in lib.ppo_last_error().decode()
    assert lib.ppo_evaluate_synth(None, x, C.byref(cfg), x, x, 2, C.byref(n), C.byref(steps)) != 0
    assert lib.ppo_evaluate_synth(x, None, C.byref(cfg), x, x, 2, C.byref(n), C.byref(steps)) != 0
    assert lib.ppo_evaluate_synth(x, x, C.byref(cfg), None, x, 2, C.byref(n), C.byref(steps)) != 0
    assert lib.ppo_evaluate_synth(x, x, C.byref(cfg), x, x, 2, None, C.byref(steps)) != 0
    assert "null argument" in lib.ppo_last_error().decode()
    assert (n.value, steps.value) == (-7, -7)
    assert lib.ppo_eval_info(None, None, 0) != 0 and "ppo_eval_info" in lib.ppo_last_error().decode()


def test_stopping_rule_under_sanitizers(tmp_path):
    """The event sort / stopping rule (csrc/ppo_eval_events.hpp, plain C++) on made-up event lists, as a
    stand-alone program built with AddressSanitizer and UBSan (tests/native/eval_events_driver.cpp)."""
    exe = str(tmp_path / "eval_events")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "ppo.cpp_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "eval_events_driver.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "eval_select: ok" in r.stdout

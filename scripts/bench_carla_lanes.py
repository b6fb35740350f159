"""Measurements of the CaRL act lanes (include/ppo_carla.h "act lanes") on one GPU; results go to stdout
and, with --out, to a file (profiles/carla/lanes.txt holds one run).

  latency   per-act host latency of ppo_carla_lane_act with one lane against the serial sequence for one
            env that the lockstep trainer runs (apps/ac_ppo_carla.cpp: four uploads from pinned memory,
            ppo_carla_rollout_act(e, e + 1), a device synchronisation, the action's copy back); the two
            arms alternate call by call. Both include one host copy of the bev row into pinned memory.
  scaling   acts per second with 1, 4 and 16 lanes driven by 16 host threads (thread i acts for env i
            through lane i % lanes, one thread per lane at a time), no env delay
  modes     collection wall time of bin/ac_ppo_carla against sixteen scripted gyms that answer an action
            after 50 ms, T = 8, once per --collect_mode; the span is taken on the gyms' side, from the
            first action received to the last state sent
"""
import argparse
import ctypes as C
import os
import statistics
import struct
import subprocess
import sys
import tempfile
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "ppo.cpp_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import ppo_amd  # noqa: E402
from ppo_amd import DeviceArray  # noqa: E402

LINES = []


def say(*a):
    s = " ".join(str(x) for x in a)
    print(s, flush=True)
    LINES.append(s)


def _agent(max_batch):
    ag = ppo_amd.CarlaAgent(max_batch=max_batch, seed=7)
    rng = np.random.default_rng(3)
    L = ag.layout2
    p = np.zeros(L.P, np.float32)
    for k in range(2, L.ntensors, 2):
        w, nw, b, nb = L.t_off[k], L.t_len[k], L.t_off[k + 1], L.t_len[k + 1]
        bound = 1.0 / np.sqrt(nw / nb)
        p[w:w + nw] = rng.uniform(-bound, bound, nw)
        p[b:b + nb] = rng.uniform(-bound, bound, nb)
    p[L.hi], p[L.lo] = 1.0, -1.0
    ag.load_params(p)
    return ag


def _obs(n):
    rng = np.random.default_rng(1)
    return (rng.integers(0, 256, (n, 15, 192, 192), dtype=np.uint8), rng.uniform(-1, 1, (n, 8)).astype(np.float32),
            rng.uniform(-1, 1, (n, 3)).astype(np.float32))


def latency(reps, warmup):
    lib = ppo_amd.lib()
    hip = C.CDLL("libamdhip64.so")
    ag = _agent(2)
    ro = ppo_amd.CarlaRollout(ag, 2, 1, 1, 1)
    lane = ro.lane()
    bev, meas, vmeas = _obs(1)
    nb = bev[0].nbytes
    # the lockstep trainer's buffers: pinned host and device copies of the next observation
    h_bev, h_f = C.c_void_p(), C.c_void_p()
    assert hip.hipHostMalloc(C.byref(h_bev), C.c_size_t(nb), 0) == 0
    assert hip.hipHostMalloc(C.byref(h_f), C.c_size_t(64 * 4), 0) == 0
    d_bev, d_meas, d_vmeas, d_done, d_act = (DeviceArray((nb,), np.uint8), DeviceArray(8), DeviceArray(3), DeviceArray(1),
                                             DeviceArray(2))
    hf = (C.c_float * 64).from_address(h_f.value)
    hf[0:8] = list(meas[0])
    hf[8:11] = list(vmeas[0])
    hf[11] = 0.0
    act = np.zeros(2, np.float32)

    def serial():
        C.memmove(h_bev.value, bev.ctypes.data, nb)  # put_obs
        lib.ppo_memcpy_h2d(d_bev.ptr, h_bev.value, nb)
        lib.ppo_memcpy_h2d(d_meas.ptr, h_f.value, 32)
        lib.ppo_memcpy_h2d(d_vmeas.ptr, h_f.value + 32, 12)
        lib.ppo_memcpy_h2d(d_done.ptr, h_f.value + 44, 4)
        rc = lib.ppo_carla_rollout_act(ro._h, 0, 0, 1, d_bev.ptr, d_meas.ptr, d_vmeas.ptr, d_done.ptr, d_act.ptr, None)
        lib.ppo_device_sync()
        lib.ppo_memcpy_d2h(h_f.value + 48, d_act.ptr, 8)
        return rc

    def laned():
        return lib.ppo_carla_lane_act(lane._h, 1, 0, bev.ctypes.data, meas.ctypes.data, vmeas.ctypes.data, 0.0,
                                      act.ctypes.data)

    ts, tl = [], []
    for i in range(warmup + reps):
        t0 = time.perf_counter()
        assert serial() == 0
        t1 = time.perf_counter()
        assert laned() == 0
        t2 = time.perf_counter()
        if i >= warmup:
            ts.append(t1 - t0)
            tl.append(t2 - t1)
    us = lambda v: f"{1e6 * v:8.1f}"  # noqa: E731
    say(f"latency per act, one env, {reps} alternating repetitions after {warmup} warm-up (host clock, us)")
    say(f"  serial sequence (4 uploads + rollout_act + device sync + D2H): median {us(statistics.median(ts))}  "
        f"mean {us(statistics.fmean(ts))}  min {us(min(ts))}")
    say(f"  ppo_carla_lane_act, one lane:                                 median {us(statistics.median(tl))}  "
        f"mean {us(statistics.fmean(tl))}  min {us(min(tl))}")
    say(f"  lane / serial (medians): {statistics.median(tl) / statistics.median(ts):.3f}")
    ro.close(), ag.close()
    hip.hipHostFree(h_bev), hip.hipHostFree(h_f)


def scaling(acts_per_thread):
    lib = ppo_amd.lib()
    nthreads = 16
    ag = _agent(16)
    ro = ppo_amd.CarlaRollout(ag, 1, nthreads, 1, 1)
    bev, meas, vmeas = _obs(nthreads)
    say(f"acts per second, {nthreads} host threads, {acts_per_thread} acts each, no env delay")
    base = None
    for nl in (1, 4, 16):
        lanes = [ro.lane() for _ in range(nl)]
        locks = [threading.Lock() for _ in range(nl)]
        start = threading.Barrier(nthreads + 1)
        errors = []

        def work(i):
            out = np.zeros(2, np.float32)
            ln, lk = lanes[i % nl], locks[i % nl]
            start.wait()
            for _ in range(acts_per_thread):
                with lk:
                    rc = lib.ppo_carla_lane_act(ln._h, 0, i, bev[i].ctypes.data, meas[i].ctypes.data,
                                                vmeas[i].ctypes.data, 0.0, out.ctypes.data)
                if rc:
                    errors.append(lib.ppo_last_error().decode())
                    return

        for _ in range(2):  # the first pass warms the lanes up
            ths = [threading.Thread(target=work, args=(i,)) for i in range(nthreads)]
            for t in ths:
                t.start()
            start.wait()
            t0 = time.perf_counter()
            for t in ths:
                t.join()
            dt = time.perf_counter() - t0
            assert not errors, errors
        rate = nthreads * acts_per_thread / dt
        base = base or rate
        say(f"  {nl:2d} lane(s): {rate:9.0f} acts/s  ({1e6 * dt / (nthreads * acts_per_thread):7.1f} us per act overall, "
            f"x{rate / base:.2f} of one lane)")
        for ln in lanes:
            ln.close()
        ro._lanes = []
    ro.close(), ag.close()


def modes(delay, steps):
    from zmtp_peer import Peer
    app = os.path.join(ROOT, "ppo.cpp_amd", "bin", "ac_ppo_carla")
    ports = list(range(6121, 6137))
    nbytes = 15 * 192 * 192

    def gym(comm, port, held):
        try:
            rng = np.random.default_rng(port)
            states = [rng.integers(0, 256, nbytes, dtype=np.uint8).tobytes() for _ in range(4)]  # reused: less GIL time
            conf = Peer.connect("PAIR", f"ipc://{comm}/comm_files/{port}.conf_lock", timeout=120)
            conf.recv()
            conf.send([b"config received"])
            env = Peer.connect("PAIR", f"ipc://{comm}/comm_files/{port}.lock", timeout=120)
            env.send([b"Connected to leaderboard gym."])
            k = 0

            def state(k):
                return [states[k % 4], rng.uniform(-1, 1, 8).astype(np.float32).tobytes(),
                        rng.uniform(-1, 1, 3).astype(np.float32).tobytes(), struct.pack("<f", 0.5), b"\x00", b"\x00",
                        struct.pack("<i", k), struct.pack("<i", 0)]

            env.send(state(k))
            while True:
                env.recv()
                t0 = time.monotonic()
                time.sleep(delay)
                k += 1
                env.send(state(k))
                held.append((t0, time.monotonic()))
        except (ConnectionError, BrokenPipeError, OSError):
            pass

    say(f"collection wall time of bin/ac_ppo_carla, {len(ports)} scripted gyms answering after {1e3 * delay:.0f} ms, "
        f"T = {steps}, one iteration (first action received to last state sent, gym side)")
    span = {}
    for mode in ("lockstep", "threads"):
        with tempfile.TemporaryDirectory() as d:
            comm, held = os.path.join(d, "team_code"), []
            gyms = [threading.Thread(target=gym, args=(comm, p, held), daemon=True) for p in ports]
            for g in gyms:
                g.start()
            cmd = [app, "--team_code_folder", comm, "--logdir", os.path.join(d, "logs"), "--exp_name", mode, "--num_envs",
                   str(len(ports)), "--num_steps", str(steps), "--num_minibatches", "2", "--update_epochs", "1",
                   "--total_timesteps", str(steps * len(ports)), "--collect_mode", mode]
            for p in ports:
                cmd += ["--ports", str(p)]
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
            for g in gyms:
                g.join(timeout=10)
            assert res.returncode == 0, (res.stdout[-1000:], res.stderr[-1000:])
            assert len(held) == steps * len(ports), len(held)
            span[mode] = max(t1 for _, t1 in held) - min(t0 for t0, _ in held)
            say(f"  {mode:8s}: {span[mode]:7.3f} s  ({steps * len(ports)} env steps; the delays alone: "
                f"{steps * len(ports) * delay if mode == 'lockstep' else steps * delay:.2f} s)")
    say(f"  lockstep / threads: {span['lockstep'] / span['threads']:.2f}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="*", default=["latency", "scaling", "modes"])
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--acts", type=int, default=100)
    ap.add_argument("--delay", type=float, default=0.05)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ppo_amd.set_device(0)
    if "latency" in a.what:
        latency(a.reps, a.warmup)
    if "scaling" in a.what:
        scaling(a.acts)
    if "modes" in a.what:
        modes(a.delay, a.steps)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")

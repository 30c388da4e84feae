"""The CUs k_fft_r32's grid leaves free (host/batch_plan.h fft_reserve_cus, SDR_FFT_RESERVE): the grid is any size from
one workgroup to one per CU, and the kernel's frame claiming and its finishing count (the launch's last workgroup puts the
band's counters back to zero) must hold for every one of them.  The check is tests/test_fft_r32_stealing.py's: frame f of
a batch is frame f % 61 of a pool of random frames, and every psd row must be bit-equal to the CPU oracle's.

  forced reserves   1, the rule's value at config 3 (8192-frame batches), CUs - 1 (a grid of one workgroup) and beyond the
                    CU count (clamped to one workgroup); 1024 and then 1031 frames on one bank - the second batch finds
                    the counters its predecessor reset, under a grid that does not divide the batch
  three bands       350 frames each, (CUs - reserve) not a multiple of three
  graph replays     two replays of 1024-frame batches under a forced reserve
  queue probe       one hardware queue in the process: the bank finds its streams on a shared queue (a process of its own)
  end to end        the default rule at the smallest batch length at which plan_batch reserves, 8 listeners, through
                    sdr_poll against the oracle: frame records, peaks, edges, runes (tests/test_gpu_parity_bench_sizes.py)
"""
import os
import re

import pytest

from parity_case import Case
from parity_tools import capi, check_pool_rows, pool_bank, pool_batch, pool_frames  # noqa: F401 (capi: the fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN_H = open(os.path.join(ROOT, "sdrainer_amd", "csrc", "host", "batch_plan.h")).read()


def _const(name):
    return int(re.search(r"constexpr int %s = (\d+);" % name, PLAN_H).group(1))


def rule_reserve(n_frames, n_bands=1):
    """fft_reserve_cus for a noise-scan batch of N = 16384 that starts a cumulation (tests/host/test_batch_plan_reserve.cpp
    pins the C++ rule itself; this restates it to name config 3's value)."""
    if n_frames * n_bands < _const("kReserveMinFrames"):
        return 0
    slots = -(-n_frames // 100)
    parts = 2 if slots * n_bands < 64 else 1
    wgs = slots * parts * n_bands
    return min(_const("kReserveMax"), -(-wgs // _const("kReserveRounds")) + _const("kReserveExtra"))


@pytest.fixture(scope="module")
def cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def pools():
    """The pools every case shares: (iq, oracle psd) by index."""
    return [pool_frames(7600 + i) for i in range(3)]


@pytest.mark.parametrize("which", ["one", "rule", "all_but_one", "beyond"])
def test_forced_reserve(capi, cus, pools, monkeypatch, which):
    import torch
    reserve = {"one": 1, "rule": rule_reserve(8192), "all_but_one": cus - 1, "beyond": cus + 40}[which]
    assert reserve > 0
    monkeypatch.setenv("SDR_FFT_RESERVE", str(reserve))
    bank = pool_bank(capi, 1, 1031)
    for i, frames in enumerate([1024, 1031]):
        iq, want = pools[i]
        dev = pool_batch(torch.from_numpy(iq).cuda(), frames)
        torch.cuda.synchronize()
        bank.process_device(dev.data_ptr(), frames)
        bank.sync()
        check_pool_rows(bank, 0, frames, want)
    bank.close()


def test_three_bands(capi, cus, pools, monkeypatch):
    """ceil((CUs - reserve) / 3) workgroups per band, the division not exact."""
    import torch
    reserve = 40 if (cus - 40) % 3 else 41
    assert (cus - reserve) % 3 != 0
    monkeypatch.setenv("SDR_FFT_RESERVE", str(reserve))
    frames = 350
    bank = pool_bank(capi, 3, frames)
    dev = torch.stack([pool_batch(torch.from_numpy(pools[b][0]).cuda(), frames) for b in range(3)]).contiguous()
    torch.cuda.synchronize()
    bank.process_device(dev.data_ptr(), frames)
    bank.sync()
    for b in range(3):
        check_pool_rows(bank, b, frames, pools[b][1])
    bank.close()


def test_graph_replays(capi, pools, monkeypatch):
    """The captured launch keeps the reserve of its capture; the counters' reset needs no host step."""
    import torch
    monkeypatch.setenv("SDR_FFT_RESERVE", "48")
    per = 1024
    bank = pool_bank(capi, 1, per)
    stream = torch.cuda.Stream()
    bank.set_stream(stream.cuda_stream)
    K = bank.graph_batches
    bank.graph_capture(per)
    for rep in range(2):
        use = [pools[(rep + k) % len(pools)] for k in range(K)]
        devs = [pool_batch(torch.from_numpy(p[0]).cuda(), per) for p in use]
        torch.cuda.synchronize()
        bank.graph_launch([d.data_ptr() for d in devs])
        bank.sync()
        check_pool_rows(bank, 0, per, use[-1][1])  # (the read calls see the replay's last batch)
    bank.graph_release()
    bank.close()


def test_default_rule_end_to_end(capi, monkeypatch):
    """No switch set: one batch of the smallest length at which the plan reserves, 8 listeners, delivered through sdr_poll."""
    monkeypatch.delenv("SDR_FFT_RESERVE", raising=False)
    frames = _const("kReserveMinFrames")
    assert rule_reserve(frames) > 0 and rule_reserve(frames - 1) == 0
    Case(16384, 1, 8, 8, [("batch", frames)], seed=3700).run(capi).close()


def _probe_case(extra_env):
    import subprocess
    import sys
    env = dict(os.environ, SDR_QUEUE_DEBUG="1", **extra_env)
    env.pop("SDR_FFT_RESERVE", None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "queue_probe_case.py")], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    reports = [l for l in p.stderr.splitlines() if l.startswith("sdr: FFT stream")]
    return reports, p.stdout.strip().splitlines()[-1]


def test_queue_probe_finds_a_shared_queue():
    """The reserve pays only where the FFT's stream has a hardware queue that none of the bank's streams uses; the bank
    looks at sdr_create and at sdr_set_stream (capi_bank.hip probe_fft_queue).  With ONE hardware queue in the process every
    stream shares it: both looks must say so, and the batch - planned without a reserve then - is the oracle's.  With the
    runtime's default queues the probe reports too, whatever it finds, and the rows are the same."""
    one, rows_one = _probe_case({"GPU_MAX_HW_QUEUES": "1"})
    assert len(one) == 2 and all("SHARES" in l for l in one), one
    assert rows_one.startswith("rows differing from the oracle: 0,"), rows_one
    default, rows_default = _probe_case({})
    assert len(default) == 2, default
    assert rows_default == rows_one

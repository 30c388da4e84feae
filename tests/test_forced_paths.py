"""Two stages have two implementations and the launch picks by batch geometry: the cumulation (every slot exact for short
batches; an upper bound of every completed cumulation + the exact value only where FindPeaks looks, from 64 M samples per
batch on: k_peaks.hip) and FindNoiseFloor's variance chains (the float64 matrix pipe for short batches, two vector-ALU
chain groups per workgroup for long ones: k_noise.hip).  The parity tests run each at the sizes that pick it; here each is
FORCED onto the sizes that would not (SDR_CUM_BOUND / SDR_VAR_MFMA), in a process of its own, so that carries, partial
slots, nine-window geometries, batch splits and the bench-size batches all go through both.

Round 5: FindNoiseFloor has two paths as well - the one-pass scan with values certified where they are consumed
(k_noise_scan.hip, noise_cert.h; the default) and the ordered chains of rounds 1-4 (SDR_NOISE_PATH=chains).  The chains run
the same parity tests here; and the scan is run with its literal fallback FORCED for every frame and for every third one
(SDR_NOISE_FORCE_EXACT), so that the list of flagged frames, the exact kernel behind it and the mix of both are exercised
(a frame is flagged by itself about three times in 10^5)."""
import os
import re
import subprocess
import sys

import pytest

import fuzz_paths_gen
import peak_shape_gen
import value_range_gen

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ("test_receiver_run_bit_exact or test_nine_window_geometry or test_config5_geometry or test_batch_split_invariance_and_carry"
         " or test_scan_segment_geometries")
FUZZ_PATHS = "test_random_paths and (" + " or ".join(f"seed{s:03d}-" for s in fuzz_paths_gen.forced_selection()) + ")"
# the N = 512 cases of every value-range regime and k_fft_r32's floor and carrier_inf cases (tests/value_range_gen.py), by
# node id: a -k expression matches substrings, of the module's name and of other tests' ids too
VALUE_RANGE_FILES = [f"tests/test_value_range_gpu.py::test_value_range[{i}]" for i in value_range_gen.FORCED]
VALUE_RANGE = ""
# the peak scan at word, span and row ends and at its capacities (tests/peak_shape_gen.py), by node id: the whole module, and
# its N = 16384 rows
PEAK_SHAPE_FILES = list(peak_shape_gen.NODE_IDS)
PEAK_SHAPE_16384 = list(peak_shape_gen.NODE_IDS_16384)


@pytest.mark.parametrize("env, files, sel", [
    ({"SDR_CUM_BOUND": "1", "SDR_VAR_MFMA": "0"}, ["tests/test_gpu_parity.py", "tests/test_dsp_golden.py"], SMALL + " or golden"),
    ({"SDR_CUM_BOUND": "0", "SDR_VAR_MFMA": "1"}, ["tests/test_gpu_parity_bench_sizes.py"], "config3 or config5 or config2"),
    ({"SDR_NOISE_PATH": "chains"}, ["tests/test_gpu_parity.py", "tests/test_dsp_golden.py", "tests/test_gpu_parity_bench_sizes.py"],
     SMALL + " or golden or config3 or config2"),
    ({"SDR_NOISE_PATH": "chains", "SDR_CUM_BOUND": "1", "SDR_VAR_MFMA": "0"}, ["tests/test_gpu_parity.py"], SMALL),
    ({"SDR_NOISE_FORCE_EXACT": "1"}, ["tests/test_gpu_parity.py", "tests/test_dsp_golden.py"], SMALL + " or golden"),
    ({"SDR_NOISE_FORCE_EXACT": "3", "SDR_CUM_BOUND": "1"}, ["tests/test_gpu_parity.py", "tests/test_gpu_parity_bench_sizes.py"],
     SMALL + " or config5 or config2"),
    # the randomised streams and cuts of the fuzz test through the cumulation's bound-and-refine path and the wide
    # refinement workgroups (its batches are far too short to pick either by themselves: round 4's advice)
    # k_fft_r32 and its wide tap on batches far too short to pick them, under the bound-and-refine path: listeners'
    # columns from the wide tap, a signal without a listener from the psd array, both refinement shapes
    ({"SDR_FFT_R32": "1", "SDR_CUM_BOUND": "1", "SDR_REFINE_WIDE": "1"}, ["tests/test_gpu_parity.py"], "test_scan_segment_geometries"),
    ({"SDR_FFT_R32": "1", "SDR_CUM_BOUND": "1", "SDR_REFINE_WIDE": "0"}, ["tests/test_gpu_parity.py"], "test_scan_segment_geometries"),
    ({"SDR_FFT_R32": "1", "SDR_CUM_BOUND": "1", "SDR_FUZZ_N": "16384", "SDR_FUZZ_SEEDS": "6"}, ["tests/test_gpu_fuzz.py"], "random_streams"),
    # config 3's 256 listeners x 2048 frames with the bound forced on: the refinement reads 768 columns per cumulation from
    # the wide tap, and the peaks are the oracle's
    ({"SDR_CUM_BOUND": "1"}, ["tests/test_gpu_parity_bench_sizes.py"], "config3"),
    ({"SDR_CUM_BOUND": "1", "SDR_REFINE_WIDE": "1"}, ["tests/test_gpu_fuzz.py"], "random_streams"),
    ({"SDR_CUM_BOUND": "1", "SDR_REFINE_WIDE": "0", "SDR_NOISE_PATH": "chains", "SDR_VAR_MFMA": "0"}, ["tests/test_gpu_fuzz.py"], "random_streams"),
    # seeds of the path fuzz that between them reach every FFT kernel family, input path and adversarial kind
    # (fuzz_paths_gen.forced_selection), through bound-and-refine in both refinement shapes and through the chains
    ({"SDR_CUM_BOUND": "1", "SDR_REFINE_WIDE": "0"}, ["tests/test_gpu_fuzz_paths.py"], FUZZ_PATHS),
    ({"SDR_CUM_BOUND": "1", "SDR_REFINE_WIDE": "1"}, ["tests/test_gpu_fuzz_paths.py"], FUZZ_PATHS),
    ({"SDR_NOISE_PATH": "chains"}, ["tests/test_gpu_fuzz_paths.py"], FUZZ_PATHS),
    # psd words across the whole float32 range (subnormal, zero among subnormals, +Inf at carriers, in the noise, everywhere,
    # 670 dB within a cumulation): the scan's literal fallback on these rows, the chains with both variance kernels, and the
    # bound kernels on their floor_hw and `special` branches in both refinement shapes
    ({"SDR_NOISE_FORCE_EXACT": "1"}, VALUE_RANGE_FILES, VALUE_RANGE),
    ({"SDR_NOISE_FORCE_EXACT": "3"}, VALUE_RANGE_FILES, VALUE_RANGE),
    ({"SDR_NOISE_PATH": "chains"}, VALUE_RANGE_FILES, VALUE_RANGE),
    ({"SDR_NOISE_PATH": "chains", "SDR_VAR_MFMA": "1"}, VALUE_RANGE_FILES, VALUE_RANGE),
    ({"SDR_CUM_BOUND": "1", "SDR_REFINE_WIDE": "0"}, VALUE_RANGE_FILES, VALUE_RANGE),
    ({"SDR_CUM_BOUND": "1", "SDR_REFINE_WIDE": "1"}, VALUE_RANGE_FILES, VALUE_RANGE),
    # runs at word, span and row ends, runs longer than a word, tied pairs across every word end and more runs than max_peaks:
    # by default these short batches take Refine::NONE - here through k_cum_bound and k_cum_refine's halo terms in both
    # refinement shapes, and at N = 16384 behind k_fft_r32, whose wide tap then serves the listener rows' columns
    ({"SDR_CUM_BOUND": "1", "SDR_REFINE_WIDE": "0"}, PEAK_SHAPE_FILES, ""),
    ({"SDR_CUM_BOUND": "1", "SDR_REFINE_WIDE": "1"}, PEAK_SHAPE_FILES, ""),
    ({"SDR_FFT_R32": "1", "SDR_CUM_BOUND": "1", "SDR_REFINE_WIDE": "0"}, PEAK_SHAPE_16384, ""),
    ({"SDR_FFT_R32": "1", "SDR_CUM_BOUND": "1", "SDR_REFINE_WIDE": "1"}, PEAK_SHAPE_16384, ""),
])
def test_parity_with_the_other_implementation_forced(env, files, sel):
    p = subprocess.run([sys.executable, "-m", "pytest", *[os.path.join(ROOT, f) for f in files], "-q", "-x", "-m", "gpu", "-k", sel,
                        "-p", "no:cacheprovider"], env=dict(os.environ, **env), cwd=ROOT, capture_output=True, text=True, timeout=1200)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-2000:]
    assert " passed" in p.stdout and "failed" not in p.stdout
    if files is VALUE_RANGE_FILES:  # exactly the cases named, none deselected and none besides
        assert len(files) == 10 and re.search(r"(^|\s)10 passed", p.stdout) and "deselected" not in p.stdout, p.stdout[-3000:]
    if files is PEAK_SHAPE_FILES or files is PEAK_SHAPE_16384:
        assert len(files) == (32 if files is PEAK_SHAPE_FILES else 5), len(files)
        assert re.search(rf"(^|\s){len(files)} passed", p.stdout) and "deselected" not in p.stdout, p.stdout[-3000:]

"""The host halves of the one-shot units under the sanitizers (CPU only, no GPU and no Python in the checked process)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gaussian_process_transportation_amd", "csrc")


def test_oneshot_host_orchestration_under_sanitizers():
    """`make host-oneshot-asan` compiles gpt_batch_host.hip, gpt_select_host.hip, gpt_svgp_train_host.hip, gpt_svgp_surface_host.hip
    and gpt_api.hip with g++ -fsanitize=address,undefined against csrc/host_stub/ into a program with its own main
    (host_stub/oneshot_driver.cpp).  It calls the real entry points on malloc'ed "device" memory: the stand-in launchers walk what
    the kernels would read and write, with every offset and size derived from the launch arguments as the kernels derive them, so a
    mistake in the packing of the batch images (the int tails of the int64 and double images, odd and even B), in the offsets of
    the outputs, in the row padding and the eleven buffers of the selection, in the theta layouts, the per-task workspace stride,
    the schedule offset by batch_begin[0], or in the sixteen buffers of the surface prediction (M = 1, 64, 65 and
    SF_PRED_CHUNK + 1 = 1025: the panels are 4 MiB each) is a sanitizer report here and not a fault on a GPU.  Outputs start as
    sentinels: what was not asked for, a failed batch member's slices and the outputs of a failed call must keep them; after
    every call no allocation, stream or event may be left.  Also gpt_inverse_map's hand-carved image (gpt_fit at N = 5, then
    M = 1 and 3 with the optional arrays present and absent)."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    subprocess.run(["make", "-C", CSRC, "host-oneshot-asan"], check=True, capture_output=True)
    env = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(CSRC, "build", "gpt_host_oneshot_asan")], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "ONESHOT_DRIVER_OK" in r.stdout, (r.stdout[-1500:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]

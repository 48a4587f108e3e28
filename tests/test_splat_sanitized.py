"""The host code of the point-cloud camera under AddressSanitizer and UndefinedBehaviorSanitizer - no GPU, and nothing is added to the
environment (the executable carries the sanitizers' runtime itself): a stand-alone C program with its own main
(examples/c_host/splat_eval.c) is linked with the host halves of csrc/fpv_hip.hip, csrc/fpv_detect.hip and csrc/fpv_splat.hip, all
built with -fsanitize=address,undefined, and run.  It derives a 16 x 12 camera and the clouds of a ground, 70 cylinders and a gate,
and evaluates a few drones into exactly sized heap buffers with a padded image_ld and point_ld (NaN in the points' padding) - one
object and the full 72, an object without points, all three encodings, with and without the centroid - and returns 0 when every
check holds and no sanitizer spoke."""
import os
import subprocess

from conftest import REPO

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SAN = "-fsanitize=address,undefined"


def test_splat_derive_cloud_derive_and_splat_eval_run_clean_under_asan_and_ubsan(tmp_path):
    lib_o, det_o, unit_o, main_o, exe = (str(tmp_path / f) for f in ("fpv_host.o", "fpv_detect.o", "fpv_splat.o", "splat_eval.o", "splat_eval"))
    run = lambda cmd: subprocess.run(cmd, check=True, capture_output=True, text=True)  # noqa: E731
    clang = run([HIPCC, "--print-prog-name=clang"]).stdout.strip()          # the C compiler hipcc drives: no compiler, no pass
    assert os.path.isfile(clang), clang
    for src, obj in (("fpv_hip.hip", lib_o), ("fpv_detect.hip", det_o), ("fpv_splat.hip", unit_o)):
        run([HIPCC, "--offload-arch=gfx950", "-O1", "-Xarch_host", SAN, "-Xarch_host", "-fno-sanitize-recover=undefined", "-ffp-contract=off",
             "-std=c++17", "-c", os.path.join(REPO, "fpyv_amd", "csrc", src), "-o", obj])
    run([clang, "-O1", "-g", SAN, "-fno-sanitize-recover=undefined", "-I" + os.path.join(REPO, "include"), "-c",
         os.path.join(REPO, "examples", "c_host", "splat_eval.c"), "-o", main_o])
    run([HIPCC, SAN, lib_o, det_o, unit_o, main_o, "-o", exe])
    env = {k: v for k, v in os.environ.items() if k not in ("ASAN_OPTIONS", "UBSAN_OPTIONS")}      # the sanitizers' defaults
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "FAILED" not in r.stdout and r.stdout.count("ok:") == 17 and "0 failures" in r.stdout
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    # the program really carries the sanitizer's runtime
    assert b"__asan_init" in open(exe, "rb").read()

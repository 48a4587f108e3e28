"""The host code of the pursuit task under AddressSanitizer and UndefinedBehaviorSanitizer - no GPU, and nothing is added to the
environment (the executable carries the sanitizers' runtime itself): a stand-alone C program with its own main
(examples/c_host/pursuit_eval.c) is linked with the host halves of csrc/fpv_hip.hip, csrc/fpv_chase.hip and csrc/fpv_pursuit.hip, all
built with -fsanitize=address,undefined, and run.  It fills the path table, draws a respawn, evaluates a reset call with a mask, steps
that capture and respawn, and a step with the guidance law into exactly sized heap buffers with padded rows, and returns 0 when
every check holds and no sanitizer spoke."""
import os
import subprocess

from conftest import REPO

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SAN = "-fsanitize=address,undefined"


def test_pursuit_derive_sample_and_eval_run_clean_under_asan_and_ubsan(tmp_path):
    units = [("fpv_hip.hip", "fpv_host.o"), ("fpv_chase.hip", "fpv_chase.o"), ("fpv_pursuit.hip", "fpv_pursuit.o")]
    objs = [str(tmp_path / o) for _, o in units]
    main_o, exe = str(tmp_path / "pursuit_eval.o"), str(tmp_path / "pursuit_eval")
    run = lambda cmd: subprocess.run(cmd, check=True, capture_output=True, text=True)  # noqa: E731
    clang = run([HIPCC, "--print-prog-name=clang"]).stdout.strip()          # the C compiler hipcc drives: no compiler, no pass
    assert os.path.isfile(clang), clang
    for (src, _), obj in zip(units, objs):
        run([HIPCC, "--offload-arch=gfx950", "-O1", "-Xarch_host", SAN, "-Xarch_host", "-fno-sanitize-recover=undefined", "-ffp-contract=off",
             "-std=c++17", "-c", os.path.join(REPO, "fpyv_amd", "csrc", src), "-o", obj])
    run([clang, "-O1", "-g", SAN, "-fno-sanitize-recover=undefined", "-I" + os.path.join(REPO, "include"), "-c",
         os.path.join(REPO, "examples", "c_host", "pursuit_eval.c"), "-o", main_o])
    run([HIPCC, SAN] + objs + [main_o, "-o", exe])
    env = {k: v for k, v in os.environ.items() if k not in ("ASAN_OPTIONS", "UBSAN_OPTIONS")}      # the sanitizers' defaults
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "FAILED" not in r.stdout and r.stdout.count("ok:") == 22 and "all checks hold" in r.stdout
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    # the program really carries the sanitizer's runtime
    assert b"__asan_init" in open(exe, "rb").read()

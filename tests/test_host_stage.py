"""The staging layouts of the synchronous wrappers and the shared FeatureVector validator on the
CPU: tests/host_stage_check.cpp (csrc/stage_layout.h, built with the address and undefined-
behaviour sanitizers) run as a child process."""
import subprocess


def test_host_stage_check():
    from slam_framework_amd import build
    exe = build.build_host_stage_check()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok: "), r.stdout
    assert r.stderr == "", r.stderr

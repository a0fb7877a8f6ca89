"""The host-compilable part of csrc/ransac_device.h, which the three device RANSAC solvers share:
resolve_sample<3 / 4 / 8> against a std::vector swap-and-pop over every valid draw tuple (and, for
three draws, against the closed form the Sim3 kernel used to hold), draw_in_range at the ends of
each place's range, check_draws' code and message. tests/ransac_common_check.cpp is a stand-alone
program built by g++ alone with the address and undefined-behaviour sanitizers linked statically;
it is never loaded into Python. No GPU."""
import os
import subprocess


def test_ransac_common(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "ransac_common_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                    "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                    "-I", os.path.join(root, "slam_framework_amd", "csrc"),
                    os.path.join(root, "tests", "ransac_common_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr

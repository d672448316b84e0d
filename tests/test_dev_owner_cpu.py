"""DevOwner (lmono_amd/csrc/dev_owner.hpp), the owner of the memory behind every C ABI handle, on the host: dev_owner_test.cpp
defines the HIP calls it makes over malloc / free, with a table of live blocks and a switch that fails the N-th call, and checks
ownership, release and both growth policies.  Built with the address and undefined-behaviour sanitizers and run as a program."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lmono_amd", "csrc")


def test_dev_owner_host_program(tmp_path):
    exe = str(tmp_path / "dev_owner_test")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Wextra", "-Werror", "-Wno-unused-function", os.path.join(CSRC, "dev_owner_test.cpp"), "-o", exe])
    run = subprocess.run([exe], text=True, capture_output=True)
    assert run.returncode == 0, run.stderr
    assert run.stdout.strip() == "dev_owner ok"

"""The host logic of the staging helper the host twins share (StagedPlanes, with_real: take_amd/csrc/tk_host.h), without
a GPU: tests/staging_host is a stand-alone program that defines the three HIP calls the helper makes over the host heap
and checks which planes are present, their byte counts, the order of allocations and copies, an empty strip set and a
failed allocation — built with the address and undefined-behaviour sanitizers, so a copy of the wrong size aborts it."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_staged_planes_host_program():
    d = os.path.join(HERE, "staging_host")
    subprocess.run(["make", "-C", d], check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    r = subprocess.run([os.path.join(d, "staging_host")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout

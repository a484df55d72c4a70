"""Ownership of device memory when an allocation fails (CPU). tests/hostsim/lifetime_main.cpp runs one scenario
over CP, multi-start and Tucker sessions on the host stand-in ops and makes the k-th allocation fail for every k;
it is a stand-alone program linked against the AddressSanitizer + UBSan build of the hostsim library, so it
carries the sanitizer runtime itself. Exit status 0: no double free, use after free, leak or undefined behaviour
at any position, every failing call returned its error code with the injected message, and every call site of
the scenario was the failing one for some k."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_allocation_failure_at_every_position():
    p = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "hostsim"), "lifetime"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(p.stdout[-6000:])
    assert p.returncode == 0, p.stdout[-6000:]
    assert "allocation positions visited" in p.stdout

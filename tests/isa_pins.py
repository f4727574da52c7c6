"""Shared by the tests that pin the kernels' machine code against the committed profiles/isa_fingerprint_*.txt files."""


def fingerprint_lines(text):
    """Output of tools/isa_fingerprint.py -> {kernel name: "n=... ops-sha=..." with single spaces}."""
    out = {}
    for line in text.splitlines():
        if " n=" in line and "ops-sha=" in line:
            name, rest = line.split(" n=", 1)
            out[name.strip()] = "n=" + " ".join(rest.split())
    return out

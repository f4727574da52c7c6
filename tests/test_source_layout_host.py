"""The layout of rtiow_amd/csrc without a GPU: one translation unit per kernel family over headers that hold only what is shared.
* no source, test program or tool needs a macro to keep rt_kernels.hpp from defining kernels twice: the one that did is gone;
* the translation units that launch no render kernel do not see it: neither rt_kernels.hpp nor rt_launch.hpp is among the files
  their compilation reads;
* splitting the files moved text and no machine code: every kernel of the library -- name, instruction counts, opcode hash, as
  tools/isa_fingerprint.py --all prints them -- is what the same tool printed on the commit before the split
  (profiles/isa_fingerprint_source_split.txt)."""
import os
import subprocess
import sys

import pytest

from isa_pins import fingerprint_lines as _fingerprint_lines

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rtiow_amd", "csrc")
NO_RENDER_KERNEL = ("rt_features.hip", "rt_trace.hip", "rt_denoise.hip", "rt_temporal.hip", "rt_adaptive.hip", "rt_selftest.hip")


def test_the_render_kernel_only_macro_is_gone():
    word = "RT_RENDER_" + "KERNEL_ONLY"                 # (spelled in two pieces: this file lies under tests/ too)
    hits = []
    for top in ("rtiow_amd", "tests", "tools", "host", "include"):
        for folder, _, names in os.walk(os.path.join(ROOT, top)):
            for name in names:
                path = os.path.join(folder, name)
                if name.endswith((".so", ".pyc", ".o", ".png", ".npy", ".npz")) or os.path.islink(path):
                    continue
                with open(path, "rb") as f:
                    if word.encode() in f.read():
                        hits.append(os.path.relpath(path, ROOT))
    assert not hits, hits


@pytest.mark.parametrize("unit", NO_RENDER_KERNEL)
@pytest.mark.parametrize("define", [(), ("-DRTIOW_CROSSCHECK_MODES",)], ids=["product", "crosscheck"])
def test_units_without_a_render_kernel_do_not_read_it(unit, define):
    run = subprocess.run(["hipcc", "-MM", "-std=c++17", "--offload-arch=gfx950", *define, "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                          os.path.join(CSRC, unit)], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    deps = {os.path.basename(d) for d in run.stdout.replace("\\\n", " ").split() if not d.endswith(":")}
    assert "rt_host.hpp" in deps and "rt_params.hpp" in deps, deps      # (the list is a real one)
    assert "rt_kernels.hpp" not in deps and "rt_launch.hpp" not in deps, sorted(deps)


def test_every_kernel_has_the_machine_code_it_had_before_the_split():
    pinned = _fingerprint_lines(open(os.path.join(ROOT, "profiles", "isa_fingerprint_source_split.txt")).read())
    assert len(pinned) == 49, len(pinned)               # 22 render kernels, 4 ray-query kernels, 23 others
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_fingerprint.py"), "--all"], capture_output=True, text=True,
                         timeout=900, cwd=ROOT)
    assert run.returncode == 0, run.stderr[-2000:]
    now = _fingerprint_lines(run.stdout)
    assert sorted(now) == sorted(pinned)                # the same kernels, by name ...
    for name in pinned:                                 # ... each with the same counts and the same opcode hash
        assert now[name] == pinned[name], (name, now[name], pinned[name])

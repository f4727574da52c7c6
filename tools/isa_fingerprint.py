#!/usr/bin/env python3
"""Static fingerprint of the product kernels' ISA (no GPU): per instantiation of a kernel, the number of instructions by class
(vector / scalar / branch / LDS / vector memory / MFMA) and a hash over the opcode sequence.  A source refactoring that is meant to
leave the machine code alone is checked with it: tools/isa_fingerprint.py > before.txt ... > after.txt; diff.
The default output lists the kernels of rt_api.hip; --frames adds, after them, the frame-batch instantiations (rt_frames.hip),
--dense the dense launch's instantiations with the capped unit-sphere redraw (rt_dense.hip), --features the first-hit feature kernel
(rt_features.hip), --trace the four instantiations of the ray-query kernel (rt_trace.hip), --shade the three kernels of the wavefront
path steps (wavefront/rt_shade.hip: a folder of its own, so --all, which is pinned to the kernels of the source split, does not list them),
--paths the seven kernels of the device path queue (wavefront/rt_paths.hip, the same folder for the same reason); --weighted, with
--paths, lists bounce_weighted_kernel too, in its place behind bounce_cone_kernel (profiles/isa_fingerprint_weighted.txt: the seven
lines of --paths are pinned by tests that count them); --pixels, with --paths, likewise lists the two kernels of the wavefront list frames and
their adaptive loop, path_begin_pixels_kernel and pass_add_listed_kernel, behind path_begin_kernel (profiles/isa_fingerprint_wavefront_pixels.txt).
--env lists bounce_env_kernel of wavefront/rt_paths.hip and nothing else of that file (profiles/isa_fingerprint_env.txt); with --paths it
stands in its place behind the other bounce kernels.
--all: every kernel of every rtiow_amd/csrc/rt_*.hip, whatever its name, sorted by name and without the s_nop padding behind its
last instruction -- so a line does not depend on which translation unit the kernel lives in, nor on whether it is the last one there
(profiles/isa_fingerprint_source_split.txt, tests/test_source_layout_host.py).  --denoise-var: the same listing for the five kernels of
denoise/rt_denoise_var.hip alone (profiles/isa_fingerprint_denoise_var.txt, tests/test_denoise_var_host.py); --temporal-var: likewise
for the two kernels of denoise/rt_temporal_var.hip (profiles/isa_fingerprint_temporal_var.txt, tests/test_temporal_var_host.py).  The other outputs count
that padding, as they always did."""
import collections, glob, hashlib, os, re, subprocess, sys
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(root, "tools"))
import isa_census as ic
args = sys.argv[1:]
defs = [a for a in args if a.startswith("-D")]
everything = "--all" in args or "--denoise-var" in args or "--temporal-var" in args      # every kernel of the sources, sorted, the padding trimmed
if "--denoise-var" in args:
    sources = ["rtiow_amd/csrc/denoise/rt_denoise_var.hip"]
elif "--temporal-var" in args:
    sources = ["rtiow_amd/csrc/denoise/rt_temporal_var.hip"]
elif everything:
    sources = sorted(os.path.relpath(p, root) for p in glob.glob(os.path.join(root, "rtiow_amd", "csrc", "rt_*.hip")))
else:
    sources = ["rtiow_amd/csrc/rt_api.hip"] + [f"rtiow_amd/csrc/rt_{flag[2:]}.hip" for flag in ("--frames", "--dense", "--features", "--trace") if flag in args]
    sources += ["rtiow_amd/csrc/wavefront/rt_shade.hip"] if "--shade" in args else []
    sources += ["rtiow_amd/csrc/wavefront/rt_paths.hip"] if "--paths" in args or "--env" in args else []
dis = "\n".join(ic.build(defs, src)[1] for src in sources)
cur, seqs = None, collections.OrderedDict()
for line in dis.splitlines():
    m = re.match(r"^([0-9a-f]+) <(\S+)>:", line)
    if m:
        cur = m.group(2)
        if cur in seqs:
            raise SystemExit(f"{cur} is defined in two translation units")
        seqs[cur] = []
        continue
    m = re.match(r"^\s+([a-z][a-z0-9_]+)\s", line)
    if m and cur:
        seqs[cur].append(m.group(1))
lines = []
env_only = not everything and "--env" in args and "--paths" not in args
for name, ops in seqs.items():
    if env_only and "bounce_env_kernel" not in name and any(k in name for k in ("path_begin", "pass_add", "bounce_", "queue_")):
        continue                                           # --env without --paths: of the path queue's file, the one kernel
    if not everything and not any(k in name for k in ("render_kernel", "resolve", "features_kernel", "trace_kernel", "camera_rays_kernel", "scatter_kernel",
                                                            "accumulate_kernel", "path_begin_kernel", "bounce_kernel", "bounce_lit_kernel", "bounce_nee_kernel", "bounce_cone_kernel", "queue_scan_kernel",
                                                            "queue_compact_kernel") + (("bounce_weighted_kernel",) if "--weighted" in args else ())
                                                           + (("path_begin_pixels_kernel", "pass_add_listed_kernel") if "--pixels" in args else ())
                                                           + (("bounce_env_kernel",) if "--env" in args else ())):
        continue
    while everything and ops and ops[-1] == "s_nop":       # the padding behind a kernel: longest behind the LAST kernel of a translation unit
        ops.pop()
    c = collections.Counter(ic.classify(o, "")[0].split()[0] for o in ops)
    dem = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip().split("(")[0]
    lines.append(f"{dem:55s} n={len(ops):5d} valu={c['valu']:5d} salu={c['salu']:5d} branch={c['branch']:4d} lds={c['lds']:4d} vmem={c['vmem']:3d} mfma={c['mfma']:3d} "
                 f"ops-sha={hashlib.sha256(' '.join(ops).encode()).hexdigest()[:12]}")
print("\n".join(sorted(lines) if everything else lines))

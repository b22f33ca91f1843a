"""The VALU slots of a rollout_pair_kernel body-wave step that compute nothing, on the compiler's own listing of the shipped source.

Every VALU instruction holds the SIMD's one VALU for a 4-clock slot, so a register copy costs a step what an FMA costs.  The body
loop's copies and integer VALU instructions (tools/isa_loops.py: vmov + valu_other) were 121 (RK4) and 41 (Euler) in the listing; with the
clamp's reciprocal formed from cos(theta) itself, trig_delta scaling its increment in place under one lane mask, and the two shared
sin / cos constants pinned in VGPRs they are 108 and 36 -- what is left sits in the blocks that run rarely (the 64-step refresh, the range
extension and its doubling loop, the clamp), plus, per step: three copies of the carried sines at the loop head, eight compares and the
exchange-slot address (profiles/rollout_hot_slots.md has the histograms and the walk of the executed path).  The bounds are those counts
plus 2.  The fp64 stream must stay inside the window test_cabi_cpu.py pins (bench.py prices the kernel with it), and the kernel at two
waves per SIMD (Euler: four) without scratch."""
import ast
import os
import re
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

KERNELS = {"rk4": "_ZN4brov19rollout_pair_kernelILi1ELi2ELi0ELb0ELb0E", "euler": "_ZN4brov19rollout_pair_kernelILi0ELi2ELi0ELb0ELb0E"}
# integrator: (vmov + valu_other of the body loop as reached, static fp64 window of body + thrust loop, VGPR budget, waves per SIMD)
REACHED = {"rk4": (108, (834, 884), 256, 2), "euler": (36, (324, 374), 128, 4)}


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    from bluerov2_dynamics_amd import _build
    asm = tmp_path_factory.mktemp("hot_slots") / "rollout.s"
    subprocess.check_call([_build.hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-DBROV2_BUILDING=1", "--offload-device-only", "-S",
                           "-o", str(asm), os.path.join(_build.CSRC, "rollout.hip")], stderr=subprocess.DEVNULL)
    return asm


@pytest.mark.parametrize("integ", ["rk4", "euler"])
def test_body_loop_non_arithmetic_valu_slots(listing, integ):
    pat = KERNELS[integ]
    out = subprocess.check_output([sys.executable, os.path.join(REPO, "tools", "isa_loops.py"), str(listing), pat], text=True)
    loops = [ast.literal_eval(l.split("):", 1)[1].strip()) for l in out.splitlines() if l.startswith("loop lines")]
    assert len(loops) >= 2, out
    body, thrust = loops[0], loops[1]
    reached, (lo, hi), vgprs, occupancy = REACHED[integ]
    slots = body.get("vmov", 0) + body.get("valu_other", 0)
    print(integ, "body loop vmov + valu_other", slots, "static f64", body["f64"] + thrust["f64"])
    assert slots <= reached + 2, out
    assert lo <= body["f64"] + thrust["f64"] <= hi, out
    assert all(l.get("acc", 0) == 0 and l.get("lane", 0) == 0 for l in (body, thrust)), out
    lines = listing.read_text().split("\n")
    k = next(i for i, l in enumerate(lines) if l.startswith(pat) and ":" in l)
    e = next(i for i in range(k, len(lines)) if lines[i].startswith(".Lfunc_end"))
    info = {m.group(1): int(m.group(2)) for m in (re.match(r"; (\w+): (\d+)", l) for l in lines[e:e + 40]) if m}
    assert info["NumVgprs"] <= vgprs and info["ScratchSize"] == 0 and info["Occupancy"] == occupancy, info


def test_lean_instantiations_keep_everything_in_registers(listing):
    """trig_delta's LEAN form (two rare regions on one lane mask) is only safe where the compiler has nothing to spill: with AGPR copies in
    the kernel it has placed one at the join of the second region ahead of the instruction that restores exec, where a wave that skipped
    the region runs it with exec = 0 and loses the value.  Every instantiation that takes the form -- rollout_pair_kernel for the
    reference vehicle (GENERIC = false): both integrators, the three layouts, both lag modes, tracked and not -- must therefore have no
    scratch and no accumulator-file move anywhere in the kernel, so that a compiler that starts to spill there fails here."""
    lines = listing.read_text().split("\n")
    starts = [(i, l.split(":")[0]) for i, l in enumerate(lines) if re.match(r"^_ZN4brov19rollout_pair_kernelILi[01]ELi[012]ELi[01]ELb[01]ELb0EEEv\w*:", l)]
    names = {n for _, n in starts}
    assert len(names) == 18, sorted(names)        # Euler: 3 layouts x tracked / not; RK4: x 2 lag modes as well
    for k, name in starts:
        e = next(i for i in range(k, len(lines)) if lines[i].startswith(".Lfunc_end"))
        info = {m.group(1): int(m.group(2)) for m in (re.match(r"; (\w+): (\d+)", l) for l in lines[e:e + 40]) if m}
        acc = [l for l in lines[k:e] if l.strip().startswith("v_accvgpr") or "scratch_" in l.split(";")[0]]
        assert info["ScratchSize"] == 0 and info["NumVgprs"] <= 256 and not acc, (name, info, acc[:3])

"""rollout_pair_kernel<RK4, TPB> (the benchmark's kernel) on the compiler's own listing: the issue slots of a step that compute
nothing.  Both waves of a SIMD share one VALU, so every register copy or address add in either time loop costs the step a slot.

    thrust loop  no copy of the control row and no copy-back of the lag bank (LagZ::advance writes it in place)
    both loops   the control loads and state stores in the saddr form (wave-uniform SGPR base + 32-bit lane offset): no 64-bit
                 VGPR address arithmetic, no flat access; the state stores need no lane mask (no v_readlane of a saved mask)

The counts are static (tools/isa_loops.py picks the loops); the fp64 stream itself is pinned by test_cabi_cpu.py."""
import os
import re
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

RK4_TPB = "_ZN4brov19rollout_pair_kernelILi1ELi2ELi0ELb0ELb0E"


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    from bluerov2_dynamics_amd import _build
    asm = tmp_path_factory.mktemp("pair_listing") / "rollout.s"
    subprocess.check_call([_build.hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-DBROV2_BUILDING=1", "--offload-device-only", "-S",
                           "-o", str(asm), os.path.join(_build.CSRC, "rollout.hip")], stderr=subprocess.DEVNULL)
    return asm


def _loops(asm, pat):
    """(body loop, thrust loop) of one pair-kernel instantiation: instruction lines, comments and labels dropped."""
    out = subprocess.check_output([sys.executable, os.path.join(REPO, "tools", "isa_loops.py"), str(asm), pat], text=True)
    spans = [tuple(int(v) for v in l.split()[2].split("-")) for l in out.splitlines() if l.startswith("loop lines")]
    assert len(spans) >= 2, out
    lines = asm.read_text().split("\n")
    i0 = next(i for i, l in enumerate(lines) if l.startswith(pat) and ":" in l)
    body = lines[i0:]
    keep = lambda a, b: [l.strip() for l in body[a:b + 1] if l.strip() and not l.strip().startswith((";", "."))]
    return keep(*spans[0]), keep(*spans[1])


def _count(loop, prefix):
    return sum(l.split()[0].startswith(prefix) for l in loop)


def test_pair_loops_carry_no_copies_of_the_control_row_or_lag_bank(listing):
    body, thrust = _loops(listing, RK4_TPB)
    # thrust wave: was 28 v_mov_b64 per step (8 for the control row, 18 to move the advanced lag bank back, 2 for compares)
    assert _count(thrust, "v_mov_b64") <= 2, [l for l in thrust if l.startswith("v_mov")]
    # both loops together: 74 before; the body wave's are mostly in its rare blocks (range extension of trig_delta)
    assert _count(body, "v_mov_b64") + _count(thrust, "v_mov_b64") <= 50


def test_pair_streams_use_scalar_bases(listing):
    body, thrust = _loops(listing, RK4_TPB)
    for loop in (body, thrust):
        assert _count(loop, "v_lshl_add_u64") == 0, [l for l in loop if l.startswith("v_lshl_add_u64")]
        assert _count(loop, "flat_") == 0
    # saddr form: data / destination, 32-bit VGPR offset, SGPR pair base (the plain form has a VGPR pair and `off`)
    load = re.compile(r"^global_load_dwordx4 v\[\d+:\d+\], v\d+, s\[\d+:\d+\]")
    store = re.compile(r"^global_store_dwordx4 v\d+, v\[\d+:\d+\], s\[\d+:\d+\]")
    loads = [l for l in thrust if l.startswith("global_load_dwordx4")]
    stores = [l for l in body if l.startswith("global_store_dwordx4")]
    assert len(loads) == 4 and all(load.match(l) for l in loads), loads           # one control row: 4 x 16 bytes per lane
    assert len(stores) == 6 and all(store.match(l) for l in stores), stores       # one state: 6 x 16 bytes per lane
    # no lane mask around the stores: the body loop neither saves one to a VGPR lane nor reads it back
    assert _count(body, "v_readlane") + _count(body, "v_writelane") == 0


def test_pair_saddr_offset_bound_matches_the_launcher():
    """pair_saddr_fits(B) in rollout.hip: the largest lane offset, pair 5 of lane 63, must fit 32 bits."""
    src = open(os.path.join(REPO, "bluerov2_dynamics_amd", "csrc", "rollout.hip")).read()
    m = re.search(r"pair_saddr_fits\(int64_t B\) \{ return B > 0 && B <= \(int64_t\)\(\(0xFFFFFFFFull - 64 \* 16\) / \(5 \* 16\)\); \}", src)
    assert m, "pair_saddr_fits changed: update this check"
    bmax = (0xFFFFFFFF - 64 * 16) // (5 * 16)
    assert 63 * 16 + 5 * 16 * bmax + 15 <= 0xFFFFFFFF < 63 * 16 + 5 * 16 * (bmax + 1) + 15 + 1024   # farthest byte; bound not loose
    assert "LAYOUT != LAYOUT_TPB || pair_saddr_fits(B)" in src                  # larger TPB batches take rollout_kernel

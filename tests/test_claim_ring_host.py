"""The dynamic sweep order without a GPU (include/bdl_order.h): the header's
declarations and the export table (additive: no ABI bump), the launch-config
knob's third order, and the host-side choice of a launch's counter pair
(bayesdll_amd/csrc/bdl_claim_ring.hpp, plain C++) driven from a stand-alone
program built with AddressSanitizer and UBSan: a stream binds its slots in
turn and then walks them as a ring, a slot never serves two streams, a launch
into a capture or a graph-node rewrite gets none (order 1) and leaves the ring
as it was, and a stream with nothing left to bind gets none."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
CSRC = os.path.join(ROOT, "bayesdll_amd", "csrc")

DRIVER = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "bdl_claim_ring.hpp"
// argv: launches as <stream>[c|r] ... ; prints the slot of each
int main(int argc, char** argv) {
  bdl::ClaimRing* ring = new bdl::ClaimRing();
  for (int i = 1; i < argc; ++i) {
    char* end = nullptr;
    const uintptr_t stream = (uintptr_t)strtoull(argv[i], &end, 10);
    printf("%d ", bdl::claim_ring_next(*ring, stream, *end == 'c', *end == 'r'));
  }
  printf("\n%d %d\n", BDL_CLAIM_SLOTS, BDL_CLAIM_SLOTS_PER_STREAM);
  delete ring;
  return 0;
}
"""


def _drive(tmp_path, launches, _built={}):
    exe = _built.get("exe")
    if exe is None:
        src = tmp_path / "ring_driver.cpp"
        src.write_text(DRIVER)
        exe = str(tmp_path / "ring_driver")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-I", INCLUDE, "-I", CSRC, str(src),
                               "-o", exe])
        _built["exe"] = exe
    out = subprocess.run([exe] + [str(x) for x in launches], check=True, capture_output=True,
                         text=True)
    assert out.stderr == ""
    slots, consts = out.stdout.strip().splitlines()
    return [int(s) for s in slots.split()], tuple(int(c) for c in consts.split())


def test_header_declares_exactly_the_three_entry_points():
    text = open(os.path.join(INCLUDE, "bdl_order.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    fns = re.findall(r"^\s*(?:int|int64_t|void|const char\*)\s+(bdl_\w+)\s*\(", code, flags=re.M)
    assert sorted(fns) == ["bdl_order_counters", "bdl_order_last", "bdl_sweep_drift"]
    assert '#include "bdl_sgmcmc.h"' in code and "BDL_ABI_VERSION" not in code  # additive


def test_export_table_and_constants_match_the_header():
    from bayesdll_amd import _lib as L
    h = L.lib()
    assert set(L.ORDER_EXPORTS) == {"bdl_order_last", "bdl_order_counters", "bdl_sweep_drift"}
    for name in L.ORDER_EXPORTS:
        assert hasattr(h, name), name
    assert h.bdl_version() == L.ABI_VERSION == 8  # additive: no version bump
    text = open(os.path.join(INCLUDE, "bdl_order.h")).read()
    macros = {k: int(v) for k, v in re.findall(r"#define (BDL_\w+) (\d+)\b", text)}
    assert macros["BDL_CLAIM_GROUPS"] == L.CLAIM_GROUPS
    assert macros["BDL_CLAIM_SLOTS"] == L.CLAIM_SLOTS
    assert macros["BDL_CLAIM_SLOTS_PER_STREAM"] == L.CLAIM_SLOTS_PER_STREAM
    assert macros["BDL_DRIFT_EVERY"] == L.DRIFT_EVERY
    assert macros["BDL_DRIFT_SAMPLES"] == L.DRIFT_SAMPLES
    # a claim block is a whole number of block iterations at every depth
    assert all(L.CLAIM_GROUPS % (256 * u) == 0 for u in (1, 2, 4))
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "bdl_step_csghmc_dyn" in mk.split("TUS :=")[1].split("DEPS")[0]
    assert "bdl_order.h" in mk.split("DEPS :=")[1].split("CFLAGS")[0]


def test_launch_config_takes_the_third_order():
    from bayesdll_amd import kernels as K
    try:
        K.set_launch_config(1, 4, 2)
        assert K.set_launch_config(3, 2, 1) == (2 << 24) | (1 << 8) | 4
        assert K.set_launch_config(2, 1, 7) == (1 << 24) | (3 << 8) | 2
        assert K.set_launch_config(0, 0, 0) == (1 << 24) | (2 << 8) | 1  # any other value: 1
        assert K.last_order()[0] in (-1, 0, 1, 2)
    finally:
        K.set_launch_config(0, 0, 0)
    assert all(c[2] in (1, 2) for c in K.AUTOTUNE_BY_METHOD["csghmc"])
    dyn = [c for c in K.AUTOTUNE_BY_METHOD["csghmc"] if c[2] == 2]
    assert sorted((b, u) for b, u, _ in dyn) == sorted(
        (b, u) for b, u, o in K.AUTOTUNE_BY_METHOD["csghmc"] if o == 1)
    assert all(c[2] != 2 for m in ("sgld", "adam") for c in K.AUTOTUNE_BY_METHOD[m])


def test_one_stream_binds_its_slots_in_turn_and_wraps(tmp_path):
    slots, (n_slots, per_stream) = _drive(tmp_path, [7] * (3 * 16 + 1))
    assert (n_slots, per_stream) == (16, 4)
    assert slots == [i % per_stream for i in range(3 * n_slots + 1)]


def test_a_slot_never_serves_two_streams_and_a_late_stream_gets_none(tmp_path):
    # four streams in turn bind four slots each; a fifth finds nothing to bind
    launches = [1, 2, 3, 4] * 8 + [5, 1, 5, 2]
    slots, (n_slots, per_stream) = _drive(tmp_path, launches)
    owner = {}
    for s, sl in zip(launches, slots):
        if s == 5:
            assert sl == -1
            continue
        assert 0 <= sl < n_slots
        assert owner.setdefault(sl, s) == s
    for s in (1, 2, 3, 4):
        mine = [sl for st, sl in zip(launches, slots) if st == s]
        assert len(set(mine)) == per_stream
        assert mine[:per_stream] == mine[per_stream:2 * per_stream]  # its own ring


def test_capture_and_redirect_get_no_slot_and_leave_the_ring_alone(tmp_path):
    slots, _ = _drive(tmp_path, ["7", "7c", "7r", "9c", "7", "9", "7c", "7"])
    assert slots == [0, -1, -1, -1, 1, 2, -1, 3]

"""CPU side of the launch-tail work (tests/test_fmt_launch_tail_gpu.py runs the kernels):
  * tools/launch_tail_listing.py follows the longest path behind the last MFMA through a loop and a branch;
  * the fixture of the parent commit's velocities holds every case."""
import os
import sys

import numpy as np

from tests.util import GOLDEN, ROOT

LISTING = """
_Z1kv:
	global_load_dwordx4 v[0:3], v[4:5], off
.LBB0_1:
	v_mfma_f32_16x16x32_f16 v[0:3], v[4:7], v[8:11], v[0:3]
	s_cbranch_scc1 .LBB0_1
	s_waitcnt vmcnt(0)
	ds_write2_b32 v1, v2, v3
	s_waitcnt lgkmcnt(0)
	s_barrier
	s_cbranch_execz .LBB0_3
	global_load_dwordx4 v[0:3], v[4:5], off
	ds_read_b128 v[0:3], v1
	s_waitcnt vmcnt(0) lgkmcnt(0)
	global_store_dwordx4 v[4:5], v[0:3], off
.LBB0_3:
	s_endpgm
	.amdhsa_kernel _Z1kv
		.amdhsa_private_segment_fixed_size 0
		.amdhsa_next_free_vgpr 182
	.end_amdhsa_kernel
"""


def test_tail_listing_tool(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import launch_tail_listing as T
    finally:
        sys.path.pop(0)
    p = tmp_path / "k.s"
    p.write_text(LISTING)
    ks = T.kernels(str(p))
    kind, path = T.tail(ks["_Z1kv"][0])
    assert kind == "mfma" and path[0].startswith("s_cbranch_scc1") and path[-1] == "s_endpgm" and len(path) == 11
    vm, lg, loads, st, ld = T.summary(path)
    assert (vm, lg, loads, st, ld) == (["0", "0"], ["0", "0"], 1, "1xds_write2_b32", "1xds_read_b128")
    assert T.descriptor(str(p))["_Z1kv"] == [182, 0]


def test_parent_velocity_fixture_holds_every_case():
    z = np.load(os.path.join(GOLDEN, "fmt_tail_parent.npz"))
    keys = {"%d_%d_%d_%s" % (p, c, way, dt) for p, c in [(0, 1), (2, 15), (10, 50)] for way in (1, 3, 4) for dt in ("fp16", "bf16", "fp32")}
    keys.add("10_50_3_fp16_full")
    assert set(z.files) == keys
    for k in z.files:
        n_prev, n_cur = (int(x) for x in k.split("_")[:2])
        assert z[k].shape == (1, n_prev + n_cur, 512 if k.endswith("full") else 128) and z[k].dtype == np.float32
        assert np.isfinite(z[k]).all() and np.abs(z[k]).max() > 0

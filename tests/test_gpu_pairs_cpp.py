"""The C++ mirror's opt-in merged dispatch (BatchVerifier::set_merge_groups, include/cpz_batch.hpp):
tests/cpp/merge_groups_test.cpp verifies one batch through the default per-group sequence and
through one cpz_verify_each_pairs_ex call and checks results and call logs against each other."""
import subprocess

import pytest

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("groups,entries", [(2, 9), (5, 40)])
def test_merged_dispatch_equals_per_group_dispatch(groups, entries):
    import build_native
    exe = build_native.build_merge_groups_test()
    r = subprocess.run([exe, str(groups), str(entries)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split()[0] == "ok" and "calls=%d->1" % groups in r.stdout, r.stdout

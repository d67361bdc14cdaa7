"""Predictor.kernel_names() against recorded names (tests/golden/kernel_names/, written by tools/dump_kernel_names.py): what every
kernel object of the matrix's programs says it launches, line for line as when the fixtures were recorded.  The outputs of the same
programs are compared with the oracle elsewhere (test_gpu_graphs.py, test_gpu_dwconv.py, test_gpu_mbv3.py, test_gpu_image_feed.py);
this pins the route each kernel object took to get them.

A change that is meant to alter a name or a route rewrites the fixtures with the tool, in the same change; a refactor never does."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("dump_kernel_names", os.path.join(ROOT, "tools", "dump_kernel_names.py"))
dump_kernel_names = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(dump_kernel_names)
ENTRIES = [e[0] for e in dump_kernel_names.entries()]


def test_fixtures_cover_the_matrix():
    assert len(ENTRIES) == len(set(ENTRIES)) == 11
    assert sorted(os.listdir(dump_kernel_names.NAMES_DIR)) == sorted(e + ".txt" for e in ENTRIES)


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ENTRIES)
def test_kernel_names_equal_snapshot(pkg, entry):
    got, want = dump_kernel_names.kernel_names(pkg, entry), dump_kernel_names.load_fixture(entry)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, "%s: line %d differs\n  named   : %s\n  recorded: %s" % (entry, i + 1, g, w)
    assert len(got) == len(want), "%s: %d instructions named, %d recorded" % (entry, len(got), len(want))

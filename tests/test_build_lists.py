"""The file lists of ogc_amd/csrc/build.py against the directory (CPU-only checks).

A source missing from SOURCES is not linked, a header missing from HEADERS leaves stale objects behind an edit, and a source of
the cell-grid searches missing from FMAD_SOURCES would evaluate the pinned distance expression one way in both libraries."""
import glob
import importlib.util
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ogc_amd", "csrc")


def _build():
    # by its path: importing the package needs the library this script builds
    spec = importlib.util.spec_from_file_location("ogc_amd_csrc_build_for_test", os.path.join(CSRC, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _names(pattern):
    return sorted(os.path.basename(p) for p in glob.glob(os.path.join(CSRC, pattern)))


def test_build_lists_match_the_source_directory():
    build = _build()
    assert sorted(build.SOURCES) == _names("*.hip")
    assert len(set(build.SOURCES)) == len(build.SOURCES)
    missing = [h for h in _names("*.h") if h not in build.HEADERS]
    assert not missing, missing
    grid = [s for s in _names("*.hip")
            if re.search(r'^\s*#\s*include\s+"grid(_dev)?\.h"', open(os.path.join(CSRC, s)).read(), re.M)]
    assert grid, "no source includes grid.h: the pattern above is out of date"
    not_fmad = [s for s in grid if s not in build.FMAD_SOURCES]
    assert not not_fmad, not_fmad

"""The Python-visible surface of `_memb` is pinned: every callable of the module and of Reader, Builder and WordBatch with
its pybind11 signature (positional order, keyword names, defaults, return type) and doc text, every module constant with
its value. tests/golden/bindings_surface.txt is what tools/bindings_surface.py printed for commit f7e54ba, the last one
with all bindings in one translation unit; the split binding sources must register the same surface. No GPU: the
extension loads without one. The text is pybind11's rendering of the signatures (3.x: `typing.SupportsInt | ...`); a
pybind11 that renders them otherwise wants the file written again by the tool, from a build of the same sources.
"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'tools'))

import bindings_surface  # noqa: E402

PINNED = os.path.join(REPO, 'tests', 'golden', 'bindings_surface.txt')


def test_extension_surface_is_the_pinned_one():
    from memb_amd import _memb
    with open(PINNED) as pinned:
        want = pinned.read()
    got = bindings_surface.surface_text(_memb)
    assert got.splitlines() == want.splitlines()
    # the pin itself covers the three classes, the constructors' overload order and the constants
    assert 'Reader.__init__ ' in want and 'Overloaded function' in want
    assert 'Builder.add_words ' in want and 'WordBatch.pack ' in want
    assert 'QUERY_MATRIX_BLOCK = ' in want and 'pool_union_rows_to_device ' in want

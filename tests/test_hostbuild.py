"""CPU: tests/hk_common.py build(), the one compile step of the host harness: it recompiles when a file the compiler read has changed and not
otherwise, its dependencies are the compiler's own (the hand-written lists it replaced had missed headers), and the one combination of variants
that has no file name of its own is refused."""
import os

import pytest

import hk_adaptive
import hk_binding
import hk_common
import hk_features


def test_a_target_is_rebuilt_when_a_header_it_includes_changes_and_only_then(tmp_path):
    header, src, out = (str(tmp_path / n) for n in ("two.h", "two.cpp", "libtwo.so"))
    with open(header, "w") as f:
        f.write("inline int two() { return 2; }\n")
    with open(src, "w") as f:
        f.write('#include "two.h"\nextern "C" int twice(int x) { return two() * x; }\n')
    assert hk_common.build(src, src, out) == out
    assert os.path.realpath(header) in [os.path.realpath(d) for d in hk_common.dependencies(out)]
    built = os.stat(out).st_mtime_ns
    hk_common.build(src, src, out)
    assert os.stat(out).st_mtime_ns == built                     # up to date: not compiled again
    later = built + 10 ** 9
    os.utime(header, ns=(later, later))                          # the header is now newer than the library
    hk_common.build(src, src, out)
    assert os.stat(out).st_mtime_ns != built
    assert not [n for n in os.listdir(str(tmp_path)) if n.endswith(".tmp")]
    os.remove(out + ".d")                                        # a build that was interrupted between its two files
    assert hk_common.stale(out, src)


@pytest.mark.parametrize("module,headers", ((hk_adaptive, ("vr_tiles.h",)), (hk_features, ("host_scene.h", "env_pack.h"))), ids=("adaptive", "features"))
def test_the_derived_dependencies_hold_what_the_written_lists_missed(module, headers):
    names = [os.path.basename(d) for d in hk_common.dependencies(module.build())]
    for h in headers:
        assert h in names, (h, names)


def test_a_sanitizer_build_of_the_fast_tap_form_is_refused():
    with pytest.raises(AssertionError):
        hk_binding.build(sanitize=True, fast_tap=True)

"""vaq_amd/build.py takes every unit's dependencies from the compiler's -MD output instead of a table kept by hand:
the parser of that output, the output itself against a plain walk over the #include "..." lines, what makes an
object stale, and SOURCES against the files in vaq_amd/csrc."""
import os
import re
import shutil

import pytest

from vaq_amd import build

CSRC = build.CSRC
INCLUDE = os.path.join(build.ROOT, "include")


def test_parse_depfile_continuations_target_and_escaped_space():
    text = ("/tmp/o\\ bj/x.o: /src/x.hip \\\n"
            "  /src/a.h /src/with\\ space/b.h \\\n"
            "  /opt/inc/c.h\n")
    assert build.parse_depfile(text) == ["/src/x.hip", "/src/a.h", "/src/with space/b.h", "/opt/inc/c.h"]
    assert build.parse_depfile("x.o: only.c\n") == ["only.c"]
    assert build.parse_depfile("x.o:\n") == []
    assert build.parse_depfile("x.o: a$$b.h \\\n") == ["a$b.h"]
    assert build.parse_depfile("x.o: a.h b.h\na.h:\nb.h:\n") == ["a.h", "b.h"]  # (-MP's empty rules)


def include_closure(path):
    """Every file of csrc / include that `path` reaches through #include "..." lines, itself included."""
    seen, todo = set(), [path]
    while todo:
        f = todo.pop()
        if f in seen:
            continue
        seen.add(f)
        for name in re.findall(r'^\s*#\s*include\s+"([^"]+)"', open(f).read(), re.M):
            found = [os.path.join(d, name) for d in (os.path.dirname(f), CSRC, INCLUDE) if os.path.exists(os.path.join(d, name))]
            assert found, "%s includes %s, which is in neither csrc nor include" % (f, name)
            todo.append(os.path.realpath(found[0]))
    return seen


@pytest.fixture(scope="module")
def built(request):
    mp = pytest.MonkeyPatch()
    request.addfinalizer(mp.undo)
    for v in ("VAQHIP_LIB", "VAQ_NO_BUILD"):
        mp.delenv(v, raising=False)
    build.build_lib()


@pytest.mark.parametrize("src", build.SOURCES)
def test_depfile_names_the_include_closure(built, src):
    root = os.path.realpath(build.ROOT) + os.sep
    named = {os.path.realpath(f) for f in build.parse_depfile(open(build._obj(src) + ".d").read())}
    assert {f for f in named if f.startswith(root)} == include_closure(os.path.realpath(os.path.join(CSRC, src)))
    assert not build._obj_stale(src)


def test_obj_stale_without_depfile_and_with_a_missing_dependency(built, tmp_path, monkeypatch):
    src = "vaq_merge.hip"
    real = build._obj(src)
    monkeypatch.setattr(build, "OBJDIR", str(tmp_path))
    o = build._obj(src)
    assert os.path.dirname(o) == str(tmp_path)
    for ext in ("", ".flags", ".d"):
        shutil.copy2(real + ext, o + ext)
    assert not build._obj_stale(src)
    os.rename(o + ".d", o + ".d.away")
    assert build._obj_stale(src)
    os.rename(o + ".d.away", o + ".d")
    assert not build._obj_stale(src)
    text = open(o + ".d").read().rstrip("\n")
    with open(o + ".d", "w") as f:
        f.write(text + " \\\n  " + str(tmp_path / "gone.h").replace(" ", "\\ ") + "\n")
    assert build.parse_depfile(open(o + ".d").read())[-1] == str(tmp_path / "gone.h")
    assert build._obj_stale(src)
    (tmp_path / "gone.h").write_text("")
    os.utime(tmp_path / "gone.h", (0, 0))
    assert not build._obj_stale(src)
    os.utime(tmp_path / "gone.h")  # now: newer than the object
    assert build._obj_stale(src)


def test_sources_are_the_units_in_csrc():
    units = sorted(f for f in os.listdir(CSRC) if f.endswith((".hip", ".cpp")))
    assert sorted(build.SOURCES) == units
    assert len(set(build.SOURCES)) == len(build.SOURCES)

"""The set of built estimator launchers is written down once, in spectro_params.h's table (GLFER_LAUNCHERS16); the Makefile's
size lists say what is compiled and the library's symbols say what was.  The three must name the same launchers, ragged twins
included.  No GPU."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "glfer_amd", "csrc")


def _name(kind, logn, ragged):
    return "glfer_launch_%s%s_n%d" % (kind, "_ragged" if ragged else "", logn)


def _table():
    hdr = open(os.path.join(CSRC, "spectro_params.h")).read()
    body = re.search(r"#define GLFER_LAUNCHERS16\(X\)(.*?)\n(?!\s*X\()", hdr, re.S).group(1)
    rows = re.findall(r"X\((\w+),\s*(\w+),\s*(\d+),\s*([01])\)", body)
    assert len(rows) == body.count("X("), "an entry of the table the test cannot read"
    names = set()
    for kind, block, logn, twin in rows:
        assert block in ("S", "IQ", "CX")
        names.add(_name(kind, int(logn), False))
        if twin == "1":
            names.add(_name(kind, int(logn), True))
    assert len(names) == len(rows) + sum(r[3] == "1" for r in rows), "an entry twice"
    return names


def _makefile():
    mk = open(os.path.join(CSRC, "Makefile")).read().replace("\\\n", " ")
    var = {k: v.split() for k, v in re.findall(r"^(\w*LOGNS)\s*=\s*([\d ]+)$", mk, re.M)}
    names = set()
    for ragged, objs in ((False, re.search(r"^OBJS\s*=(.*)$", mk, re.M).group(1)),
                         (True, re.search(r"^RAGGED_OBJS\s*=(.*)$", mk, re.M).group(1))):
        # $(addprefix $(OBJDIR)/<kind>[_ragged]_n,$(addsuffix .o,$(<LIST>))): one object per size of the list
        for kind, rag, lst in re.findall(r"\$\(addprefix \$\(OBJDIR\)/(spectro16\w*?)(_ragged)?_n,\$\(addsuffix \.o,\$\((\w+)\)\)\)", objs):
            assert bool(rag) == ragged
            names.update(_name(kind, int(l), ragged) for l in var[lst])
        # spectro16y is built for N = 4096 alone: no size in the object's name
        for kind, rag in re.findall(r"\$\(OBJDIR\)/(spectro16y)(_ragged)?\.o", objs):
            assert bool(rag) == ragged
            names.add(_name(kind, 12, ragged))
    return names


def _library():
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "glfer_amd", "lib", "libglfer_hip.so")],
                         check=True, capture_output=True, text=True).stdout
    return set(re.findall(r"\b(glfer_launch_spectro16\w*_n\d+)$", out, re.M))


def test_table_makefile_and_library_name_the_same_launchers():
    table, makefile, library = _table(), _makefile(), _library()
    assert len(table) > 50, sorted(table)         # (the regexes found the table at all)
    assert table == makefile, (sorted(table - makefile), sorted(makefile - table))
    assert table == library, (sorted(table - library), sorted(library - table))

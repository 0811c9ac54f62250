"""The table of run-time knobs in DESIGN.md section 10 against the sources: every C2W_* environment name the library or the Python package reads
is a row of the table, and every row is read somewhere.  CPU tier: text only, no library call."""
import glob
import os
import re

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(HERE, "climate2weather_amd")
OWNED_ELSEWHERE = {"C2W_REUSE_BUILD", "C2W_BENCH_EXTRAS", "C2W_BENCH_KEEP_CACHE"}  # __graft_entry__.py, bench.py, bench_legs.py


def _read(path):
    with open(path) as f:
        return f.read()


def _library_names():
    names = set()
    for path in glob.glob(os.path.join(PKG, "csrc", "*")):
        names |= set(re.findall(r'getenv\(\s*"(C2W_[A-Z0-9_]+)"\s*\)', _read(path)))
    return names


def _python_names():
    names = set()
    for path in glob.glob(os.path.join(PKG, "*.py")):
        src = _read(path)
        names |= set(re.findall(r'environ\.get\(\s*"(C2W_[A-Z0-9_]+)"', src))
        names |= set(re.findall(r'environ\[\s*"(C2W_[A-Z0-9_]+)"\s*\]', src))
        names |= set(re.findall(r'"(C2W_[A-Z0-9_]+)"\s+(?:not\s+)?in\s+os\.environ', src))
        names |= set(re.findall(r'(?:getenv|environ\.setdefault|environ\.pop)\(\s*"(C2W_[A-Z0-9_]+)"', src))
    return names


def _table_names():
    """First column of the FIRST table of DESIGN.md section 10 (the retired names have a table of their own below it)."""
    design = _read(os.path.join(HERE, "DESIGN.md"))
    sec = design[design.index("## 10. Run-time knobs"):]
    rows, seen_table = [], False
    for line in sec.split("\n")[1:]:
        if line.startswith("|"):
            seen_table = True
            rows.append(line)
        elif seen_table:
            break
    assert rows[0].split("|")[1].strip() == "name" and set(rows[1]) <= set("|-"), rows[:2]
    names = []
    for row in rows[2:]:
        cell = row.split("|")[1]
        found = re.findall(r"`(C2W_[A-Z0-9_]+)`", cell)
        assert len(found) == 1, f"one name per row, got {cell!r}"
        names.append(found[0])
    assert len(names) == len(set(names)), "a name is listed twice"
    return set(names)


def test_design_table_lists_exactly_the_names_the_sources_read():
    lib, py, table = _library_names(), _python_names(), _table_names()
    assert lib and py  # the patterns still find the reads
    assert OWNED_ELSEWHERE <= table
    assert not (OWNED_ELSEWHERE & (lib | py))
    assert lib | py == table - OWNED_ELSEWHERE, (sorted((lib | py) - table), sorted(table - OWNED_ELSEWHERE - lib - py))


def test_every_library_knob_has_its_field_comment_in_knobs_h():
    reads = set(re.findall(r'getenv\(\s*"(C2W_[A-Z0-9_]+)"\s*\)', _read(os.path.join(PKG, "csrc", "conv_igemm.hip"))))
    assert reads == _library_names()  # one place reads the library's environment
    struct = _read(os.path.join(PKG, "csrc", "knobs.h"))
    struct = struct[struct.index("struct C2wKnobs {"):struct.index("};")]
    commented = set()
    for line in struct.split("\n")[1:]:
        if line.strip():
            m = re.match(r"\s+(?:bool|int) \w+;\s+// (C2W_[A-Z0-9_]+)\b", line)
            assert m, f"a field without its knob comment: {line!r}"
            commented.add(m.group(1))
    assert reads == commented, (sorted(reads - commented), sorted(commented - reads))

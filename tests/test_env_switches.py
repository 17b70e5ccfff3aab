"""The environment switches the native code reads are exactly those DESIGN.md
lists in its "Environment switches" table: a switch added to the sources
without a row, or a row left behind by a removed switch, fails here."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "xfemm_amd", "csrc")

# a name passed to getenv or to xfk_internal.h's two readers
READ = re.compile(r'\b(?:getenv|env_int|env_set)\s*\(\s*"((?:XFK|XFEMM)_[A-Z0-9_]+)"')


def names_read_by_sources():
    found = set()
    for d, _, files in os.walk(CSRC):
        for f in files:
            if f.endswith((".hip", ".cpp", ".h")):
                with open(os.path.join(d, f), errors="replace") as fh:
                    found.update(READ.findall(fh.read()))
    return found


def names_in_design_table():
    with open(os.path.join(ROOT, "DESIGN.md")) as fh:
        text = fh.read()
    section = text.split("### Environment switches", 1)[1]
    rows = []
    for line in section.splitlines()[1:]:
        if line.startswith("|"):
            rows.append(line)
        elif rows:   # the table ended
            break
    names = set()
    for row in rows[2:]:   # after the header and its rule
        names.update(re.findall(r"`((?:XFK|XFEMM)_[A-Z0-9_]+)`", row.split("|")[1]))
    return names


def test_design_table_lists_every_switch_the_sources_read():
    src, doc = names_read_by_sources(), names_in_design_table()
    assert src, "no switch found under xfemm_amd/csrc: the pattern no longer matches the sources"
    assert src == doc, "read but not in the table: %s; in the table but not read: %s" % (
        sorted(src - doc), sorted(doc - src))

"""Helpers shared by the tests that read include/oneshotdet_hip.h: the functions it declares and the section that declares one."""
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "oneshotdet_hip.h")


def code(text):
    """`text` without its comments"""
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def declared():
    """Every osd_* function the header declares, in the header's order; a name declared twice is listed twice."""
    return re.findall(r"\b(osd_[a-z0-9_]+)\s*\(", code(open(HEADER).read()))


def section_of(name):
    """The text, comments included, of the section (from one `/* ----` banner to the next) whose code declares `name`."""
    sections = re.split(r"(?=/\* -{20,}\n)", open(HEADER).read())
    found = [s for s in sections if re.search(r"\b%s\s*\(" % re.escape(name), code(s))]
    assert len(found) == 1, (name, len(found))
    return found[0]

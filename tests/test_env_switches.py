"""CPU: the NEUMAN_* environment settings the package and the library read are the ones INTEGRATION.md's settings table documents, so
that an experiment switch cannot be added or left behind without the table saying so."""
import os
import re

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NAME = r"NEUMAN_[A-Z0-9_]+"
# os.environ.get("X" / os.environ["X"] / os.getenv("X") in Python, getenv("X") in C++
READ = re.compile(r"""(?:environ(?:\.get\(|\[)|getenv\()\s*["'](""" + NAME + r""")["']""")


def _sources(top, exts=None):
    for d, _, files in os.walk(os.path.join(ROOT, top)):
        for f in sorted(files):
            if exts is None or f.endswith(exts):
                with open(os.path.join(d, f), errors="replace") as fh:
                    yield fh.read()


def library_reads():
    return {m for src in _sources("ml-neuman_amd", (".py", ".hip", ".h")) for m in READ.findall(src)}


def integration():
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        return f.read()


def test_every_setting_the_code_reads_is_in_the_table():
    reads = library_reads()
    assert {"NEUMAN_PRECISION", "NEUMAN_I8_KERNEL"} <= reads, "the pattern no longer finds the Python and C++ reads"
    table = set(re.findall(r"^\| `(" + NAME + r")` \|", integration(), re.M))
    assert not reads - table, f"read by ml-neuman_amd/ but not in INTEGRATION.md's settings table: {sorted(reads - table)}"


def test_every_documented_setting_is_still_read():
    used = library_reads() | {m for src in _sources("tools") for m in re.findall(NAME, src)}
    with open(os.path.join(ROOT, "bench.py")) as f:
        used |= set(re.findall(NAME, f.read()))
    documented = set(re.findall(NAME, integration()))
    assert not documented - used, f"documented in INTEGRATION.md but read nowhere: {sorted(documented - used)}"

"""The checks of a function's text and of a table of variables (csrc/function_text.hpp), without a GPU.

The header is plain C++ with no HIP type: a small program with its own main is built with the host compiler and
driven over the tables below, one process per case.  The expected values follow from the rules, not from the code:

  number test      a text is a constant if and only if strtod consumes at least one character and only blanks, tabs,
                   CR or LF follow; a text that is no constant leaves the value 0;
  names_identifier the C text names `id' as a whole identifier that is no member (`a.T'), is not glued to a digit
                   (`2T') and does not stand inside a string literal;
  c_identifier     a letter or an underscore, then letters, digits and underscores, of the C locale;
  table check      nvars >= 0 with both tables unless nvars == 0; then per entry, in the order of the table: a C name,
                   none of the built-in names, not a name of an earlier entry.  The first failure is reported."""
import math
import os
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "gerris-fft-particles_amd", "csrc")

PROGRAM = r"""
#include "function_text.hpp"
#include <cstdio>
#include <vector>
using namespace gfship;
// constant TEXT | names TEXT ID | cid (NAME | --null) | table NB B1 .. BNB NVARS (--null | N1 .. NNVARS)
int main (int argc, char ** argv)
{
  if (argc < 3) return 2;
  const std::string mode = argv[1];
  if (mode == "constant") {
    double value = 123.;
    const bool c = text_constant (argv[2], &value);
    printf ("%d %a\n", c ? 1 : 0, value);
  }
  else if (mode == "names" && argc == 4)
    printf ("%d\n", names_identifier (argv[2], argv[3]) ? 1 : 0);
  else if (mode == "cid")
    printf ("%d\n", c_identifier (std::string (argv[2]) == "--null" ? nullptr : argv[2]) ? 1 : 0);
  else if (mode == "table") {
    const int nb = atoi (argv[2]);
    if (argc < 4 + nb) return 2;
    const char * const * builtin = argv + 3;
    const int nvars = atoi (argv[3 + nb]);
    const bool null = argc > 4 + nb && std::string (argv[4 + nb]) == "--null";
    if (!null && nvars > 0 && argc != 4 + nb + nvars) return 2;
    const std::vector<int> vars (nvars > 0 ? nvars : 1, 0);
    const TableFault f = table_fault (nvars, null ? nullptr : argv + 4 + nb, null ? nullptr : vars.data (), builtin, nb);
    printf ("%d %d %s\n", (int) f.rule, f.q, f.name ? f.name : "-");
  }
  else
    return 2;
  return 0;
}
"""

# text -> the value strtod gives where the rule makes the text a constant, None where it does not
CONSTANTS = [
    ("1.5", 1.5), (" 2e-3\n", 2e-3), ("-0.", -0.0), ("1.5x", None), ("x", None), ("", None), ("1. ", 1.), ("1 2", None),
    ("0x10", 16.), (" ", None), ("\t3\r\n", 3.), ("1e", None), ("1e5 \t", 1e5), ("1.5 x", None), ("+.5", .5), (".", None),
    ("inf", math.inf), ("-", None),
]

# (text, id) -> named?
NAMES = [
    ("T + 2", "T", True), ("T1 + 2", "T", False), ("T + 2", "T1", False), ("2*T1", "T1", True),
    ("a.T", "T", False), ("a.T + T", "T", True), ("a . T", "T", True),      # only a `.' right before makes a member
    ("2T", "T", False), ("2*T", "T", True),
    ('printf ("T")', "T", False), ('"T" T', "T", True), ('"a" + T + "b"', "T", True),
    ('x + "T', "T", False), ('x + "', "x", True), ('"', "T", False),
    ("", "T", False), ("T", "", False),
    ("_T", "T", False), ("T_", "T", False), ("(T)", "T", True), ("sin(x)*Rad", "Rad", True), ("sin(x)*Rad", "si", False),
]

C_IDENTIFIERS = [
    (b"", False), (b"--null", False), (b"1a", False), (b"_", True), (b"_a1", True), (b"a", True), (b"a b", False),
    (b"a-b", False), (b"a\xc3\xa9", False), (b"\xe9", False), (b"a1_B", True), (b"a.b", False),
]

OK, INVALID, NO_C_NAME, BUILTIN, TWICE = range(5)
SOURCE = ["Rad", "Urelp", "Vrelp", "Wrelp", "x", "y", "z", "t"]
FEED = ["x", "y", "z", "t"]
# (builtin, nvars, names or None) -> (rule, entry, name)
TABLES = [
    (FEED, 0, None, (OK, 0, "-")),                   # nvars = 0 with null tables
    (FEED, 0, [], (OK, 0, "-")),
    (FEED, 2, None, (INVALID, 0, "-")),
    (FEED, -1, None, (INVALID, 0, "-")),
    (FEED, 2, ["T", "S"], (OK, 2, "-")),
    (FEED, 2, ["T", "x"], (BUILTIN, 1, "x")),
    (SOURCE, 1, ["Rad"], (BUILTIN, 0, "Rad")),
    (FEED, 1, ["Rad"], (OK, 1, "-")),                # the built-in names are parameters
    (SOURCE, 3, ["a", "b", "t"], (BUILTIN, 2, "t")),
    (FEED, 2, ["T", "T"], (TWICE, 1, "T")),
    (FEED, 3, ["a", "b", "a"], (TWICE, 2, "a")),
    (FEED, 2, ["x", "x"], (BUILTIN, 0, "x")),        # the first failure, in the order of the table
    (FEED, 1, ["1a"], (NO_C_NAME, 0, "-")),
    (FEED, 3, ["a", "", "a"], (NO_C_NAME, 1, "-")),
    ([], 2, ["x", "t"], (OK, 2, "-")),
]


def build(directory, flags=()):
    src, exe = os.path.join(directory, "function_text.cpp"), os.path.join(directory, "function_text")
    with open(src, "w") as f:
        f.write(PROGRAM)
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O2", "-Wall", "-Werror", *flags, "-I", CSRC, src,
                    "-o", exe], check=True, capture_output=True, text=True, timeout=120)
    return exe


def ask(exe, *args):
    args = [a if isinstance(a, bytes) else a.encode() for a in args]
    return subprocess.run([exe.encode()] + args, check=True, capture_output=True, timeout=60).stdout.decode().split()


def check_number(exe):
    for text, value in CONSTANTS:
        c, v = ask(exe, "constant", text)
        assert (c == "1") == (value is not None), text
        v, want = float.fromhex(v), 0. if value is None else value
        assert v == want and math.copysign(1., v) == math.copysign(1., want), (text, v)


def check_names_identifier(exe):
    for text, name, named in NAMES:
        assert ask(exe, "names", text, name) == ["1" if named else "0"], (text, name)


def check_c_identifier(exe):
    for name, ok in C_IDENTIFIERS:
        assert ask(exe, "cid", name) == ["1" if ok else "0"], name


def check_table(exe):
    for builtin, nvars, names, want in TABLES:
        got = ask(exe, "table", str(len(builtin)), *builtin, str(nvars), *(["--null"] if names is None else names))
        assert got == [str(want[0]), str(want[1]), want[2]], (builtin, nvars, names, got)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return build(str(tmp_path_factory.mktemp("function_text")))


def test_number(program):
    check_number(program)


def test_names_identifier(program):
    check_names_identifier(program)


def test_c_identifier(program):
    check_c_identifier(program)


def test_table(program):
    check_table(program)

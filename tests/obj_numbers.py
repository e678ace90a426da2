"""obj_numbers.py — TEST INFRASTRUCTURE: seeded generators of OBJ number tokens, face-corner tokens and padded files,
aimed at the edges of the device decode (take_amd/csrc/tk_obj.h): the boundary of the window in which the device converts
a number itself (15 / 16 significant digits, effective decimal exponent 22 / 23), the 4096-element scan tiles, the
dedup table and the status word.  Nothing here restates the device's algorithms.

The number tokens and their lists are oracle/obj_tokens.py's (the fixture generator tools/gen_obj_golden.py builds the
`number_grammar` case from them and must not depend on tests/); the corner tokens and the file builders are here.
Used by tests/test_obj_cpu.py and tests/test_gpu_obj.py.
"""
import numpy as np

from oracle.obj_tokens import (CURATED, EFFECTIVE_EXPONENTS, NEGATIVE_ZEROS, POSITIVE_ZEROS, REFUSED, REFUSED_GRAMMAR,  # noqa: F401
                               REFUSED_RANGE, SIG_DIGITS, number_token, number_tokens)


def corner_tokens(n, seed=7):
    """face-corner tokens in every form split_face_str meets, std::stoi's edges among them"""
    rng = np.random.default_rng(seed)
    edge = ["2147483647", "2147483648", "-2147483648", "-2147483649", "+2147483647", "4294967296", "4294967297", "-4294967297",
            "99999999999999999999", "-99999999999999999999", "0", "-0", "+0", "00012", "12abc", "-3x", "+4.5", "abc", "x1", "", "+", "-",
            "#", "1e3"]
    forms = ["{a}", "{a}/{b}", "{a}//{c}", "{a}/{b}/{c}", "{a}/", "{a}//", "{a}/{b}/", "{a}/{b}/{c}/{d}", "/{b}", "//{c}", "/", "//", "///",
             "{a}/{b}/{c}/", "{a}/{b}/{c}//{d}"]

    def piece():
        r = rng.random()
        if r < 0.45:
            return str(rng.choice(("", "+", "-"))) + str(int(rng.integers(0, 100000)))
        return str(rng.choice(edge))

    out = [f.format(a=a, b=b, c=c, d=d).encode() for f in forms for a, b, c, d in (("1", "2", "3", "4"), ("+1", "-2", "-0", "q"), ("abc", "1", "1", "1"), ("1", "1", "1", "abc"))]
    out += [e.encode() for e in edge if e]
    while len(out) < n:
        out.append(str(rng.choice(forms)).format(a=piece(), b=piece(), c=piece(), d=piece()).encode())
    return [t for t in out if t and not any(ch in t for ch in b" \t\n\v\f\r")]


# ---- files of an exact size ----------------------------------------------------------------------------------------
def comment(nbytes):
    """a comment line of exactly nbytes bytes (its '\\n' not counted), nbytes >= 1"""
    assert nbytes >= 1
    return b"#" + b"." * (nbytes - 1)


def pad_to_bytes(lines, total, trailing_newline=True, at=0):
    """the lines joined with '\\n' (and a last '\\n' if asked), with comment lines inserted in front of lines[at] so that
    the file has exactly `total` bytes"""
    room = total - (sum(len(l) + 1 for l in lines) - (0 if trailing_newline else 1))
    assert room >= 0, (total, room)
    pad = []
    while room > 0:  # a pad line of k bytes takes k + 1 with its '\n'; k = 0 is a blank line
        take = min(room, 100)
        pad.append(comment(take - 1) if take > 1 else b"")
        room -= take
    out = b"\n".join(list(lines[:at]) + pad + list(lines[at:]))
    out += b"\n" if trailing_newline else b""
    assert len(out) == total
    return out


def place_lines(placed, nlines, filler=(b"# pad", b"", b"   ", b"#")):
    """a file of exactly nlines lines (nlines - 1 '\\n' bytes, no trailing one): placed = {line index: line}, every other
    line a comment or a blank one"""
    assert all(0 <= i < nlines for i in placed)
    return b"\n".join(placed.get(i, filler[i % len(filler)]) for i in range(nlines))

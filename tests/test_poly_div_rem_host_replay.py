"""CPU-only: the per-lane steps of the series inverse and the general division (polyinv_step.cuh) replayed on the host.
tests/polyinv_host_replay.cpp includes the header outside hipcc and walks, lane by lane, the seed recurrence for n = 1, 2, SEED - 1,
SEED, one Newton level (whole, truncated, and on a reversed series: the divisor's case), whole small divisions through the
correlation and the remainder's product, and the index maps for m = 1, 2, 3 and q_len > m.  It prints stored words; they are compared
here with tests/poly_newton_ref.py.  The program is built and run twice: plain, and under AddressSanitizer + UBSan."""
import random

import pytest

from tests import hostprog
from tests import poly_newton_ref as nr

SEED = 64  # PINV_SEED
FIELDS = {  # PLK_FIELD_* id -> modulus
    0: 0x40000000000000000000000000000000038aa127696286c9842cafd400000001,
    1: 0x40000000000000000000000000000000038aa1276c3f59b9a14064e200000001,
    2: 0x12ab655e9a2ca55660b44d1e5c37b00159aa76fed00000010a11800000000001,
    4: 0x40000000000000000000000000000000224698fc094cf91b992d30ed00000001,
    5: 0x40000000000000000000000000000000224698fc0994a8dd8c46eb2100000001,
}


def _hex(p, vals):
    return " ".join("%064x" % w for w in nr.stored(p, vals))


def _cases():
    rng = random.Random(7)
    lines, want = [], []
    p = FIELDS[1]
    for n, lh, rev in [(1, 1, 0), (2, 2, 0), (SEED - 1, SEED + 5, 0), (SEED, 3, 0), (2 * SEED, 2 * SEED, 0), (SEED + 37, 200, 0), (SEED + 37, 50, 0),
                       (2 * SEED, 2 * SEED, 1), (SEED + 37, 200, 1), (SEED + 37, 50, 1), (5, 9, 1)]:
        h = nr.rand_poly(p, rng, lh)
        h[-1 if rev else 0] = rng.randrange(1, p)
        lines.append("inv 1 %d %d %d %s" % (rev, n, lh, _hex(p, h)))
        series = h[::-1] if rev else h
        want.append(("g", nr.stored(p, nr.inverse_series(p, series, n))))
    for fid, p in FIELDS.items():  # every field: the seed and one truncated level
        h = [p - 1] + nr.rand_poly(p, rng, 80)
        lines.append("inv %d 0 %d %d %s" % (fid, SEED + 9, len(h), _hex(p, h)))
        want.append(("g", nr.stored(p, nr.inverse_series(p, h, SEED + 9))))
    p = FIELDS[1]
    for k, m, pad in [(1, 1, 0), (1, 2, 3), (2, 3, 1), (5, 1, 2), (33, 2, 0), (3, SEED + 5, 4), (70, SEED + 1, 0), (40, 3, 2)]:
        a, b = nr.rand_poly(p, rng, k + m), nr.rand_poly(p, rng, k) + [rng.randrange(1, p)]
        lines.append("div 1 %d %d %d %s %s" % (k + m, k + 1, m + pad, _hex(p, a), _hex(p, b)))
        q, r = nr.divide(p, a, b)
        want.append(("q", nr.stored(p, q) + [0] * pad))
        want.append(("rem", nr.stored(p, r)))
    for m, q_len in [(1, 1), (2, 5), (3, 4)]:
        lines.append("maps %d %d" % (m, q_len))
        maps = [s if s < m else -1 for s in range(q_len)]
        series = [j if j < m else -1 for j in range(m + 1)] + [m - 1 - j if j < m else -1 for j in range(m + 1)]
        want.append(("maps", (maps, series, [(8 - i) % 8 for i in range(8)], [(t - m) % 8 for t in range(8)])))
    return lines, want


@pytest.mark.parametrize("flavour", [hostprog.PLAIN, hostprog.ASAN_UBSAN], ids=["plain", "sanitized"])
def test_steps_replayed_on_the_host(tmp_path, flavour):
    script = str(tmp_path / "cases.txt")
    lines, want = _cases()
    with open(script, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    got = hostprog.run(hostprog.build("tests/polyinv_host_replay.cpp", tmp_path, flavour, extra=("-Wall",)), script).strip().split("\n")
    assert len(got) == len(want)
    for line, (tag, expect) in zip(got, want):
        parts = line.split()
        assert parts[0] == tag
        if tag == "maps":
            groups = [[int(v) for v in grp.split()] for grp in line[len("maps"):].split("|")]
            assert groups == [list(g) for g in expect]
        else:
            assert [int(w, 16) for w in parts[1:]] == expect, tag

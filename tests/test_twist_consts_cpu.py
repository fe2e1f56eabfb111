"""The constant-memory table of the small-batch solve (csrc/msnap_twist_consts.h) against the literals it replaces:
tests/c_abi/twist_consts_dump.cpp, compiled with g++ alone, prints for order 7 and order 9 every constant the sweep and
recovery bodies read -- the HermiteConsts<K> literal and the value the kernel takes instead (the literal itself for an
inline operand, else a slot of the image).  Required: the two are equal BIT FOR BIT, every slot of the image is used,
no two slots of a set hold the same value, and the padding is zero."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "drone_path_planning_python_amd", "csrc")


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed for this test"
    exe = str(tmp_path_factory.mktemp("twist_consts") / "twist_consts_dump")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC,
                    os.path.join(ROOT, "tests", "c_abi", "twist_consts_dump.cpp"), "-o", exe], check=True)
    return subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()


def test_table_entries_are_the_literals_bit_for_bit(dump):
    rows = [ln.split() for ln in dump if ln[0] in "45"]
    # what the bodies read: (K-1)K/2 HSS + as many HEE, K-1 each of HSE[n][0], HEE[n][0], INVFACT, (K-1)^2 HSE,
    # K CE[m][0], K (K-1) each of CS and CE
    for K in (4, 5):
        mine = [r for r in rows if int(r[0]) == K]
        assert len(mine) == (K - 1) * K + 3 * (K - 1) + (K - 1) ** 2 + K + 2 * K * (K - 1)
    from_table = 0
    for K, name, n, m, code, lit, used in rows:
        assert lit == used, (K, name, n, m, code, lit, used)
        from_table += int(code) != 0
    assert from_table > len(rows) // 2          # (the table is in use at all)


def test_image_layout(dump):
    head = {int(ln.split()[1]): [int(x) for x in ln.split()[2:]] for ln in dump if ln.startswith("layout ")}
    image = [ln.split()[2] for ln in dump if ln.startswith("image ")]
    rows = [ln.split() for ln in dump if ln[0] in "45"]
    used = set()
    for K in (4, 5):
        n_sweep, sweep_at, n_rec, rec_at, total = head[K]
        assert total == len(image) and sweep_at % 8 == 0 and rec_at % 8 == 0
        for at, cnt, names in ((sweep_at, n_sweep, ("HSS", "HEE", "HSE")), (rec_at, n_rec, ("CS", "CE", "INVFACT"))):
            vals = image[at:at + cnt]
            assert len(set(vals)) == cnt, "a value held twice"
            codes = {int(r[4]) for r in rows if int(r[0]) == K and r[1] in names and int(r[4]) != 0}
            assert codes == set(range(1, cnt + 1)), "a slot nobody reads"
            used.update(range(at, at + cnt))
    inline = {"3fe0000000000000", "3ff0000000000000", "4000000000000000", "4010000000000000"}
    for i, v in enumerate(image):
        if i not in used:
            assert v == "0000000000000000"
        else:
            assert ("%016x" % (int(v, 16) & ~(1 << 63))) not in inline, "an inline operand in the table"

"""pick (csrc/fgx_launch.h), the one way a run-time kind becomes a template argument, on the CPU:
tests/host/pick_table.hip runs it nested as the episode ladder nests it (MP kind, controller, link
count, a bool) and flat, and prints one line per case.  The expected lines below are written from
pick's contract, not recorded from it: the callable is called once, with the tag of the first listed
value that equals the run-time value, and its result returned with err untouched; no listed value
equals it: the callable is not called, err is the miss message and the miss code is returned, through
every outer level unchanged."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

MP_NONE, MP_PROMP, MP_DMP, MP_PRODMP, MP_GIVEN = range(5)   # csrc/fgx_device.h
CTRL_PD, CTRL_VEL, CTRL_POS = range(3)


def ladder(mp, ctrl, nl, b):
    """What the four-level ladder of pick_table.hip must print for these run-time values."""
    if mp not in (MP_PROMP, MP_DMP, MP_PRODMP, MP_GIVEN):
        rc, calls, err = -1, 0, "bad mp kind"
    elif ctrl not in (CTRL_PD, CTRL_VEL, CTRL_POS):
        rc, calls, err = -1, 0, "bad ctrl_kind"
    elif nl not in (2, 5):
        rc, calls, err = -4, 0, "not instantiated"
    elif b not in (0, 1):
        rc, calls, err = -3, 0, "not a bool"
    else:   # the callable returns its tags: each is the value it was picked for
        rc, calls, err = mp * 1000 + ctrl * 100 + nl * 10 + b, 1, "untouched"
    return f"ladder mp={mp} ctrl={ctrl} nl={nl} b={b} -> rc={rc} calls={calls} err={err}"


def expected():
    want = [ladder(mp, ctrl, nl, b) for mp in (MP_PROMP, MP_DMP, MP_PRODMP, MP_GIVEN)
            for ctrl in (CTRL_PD, CTRL_VEL, CTRL_POS) for nl in (2, 5) for b in (0, 1)]
    want += [ladder(mp, CTRL_PD, 5, 0) for mp in (MP_NONE, 5, -1)]
    want += [ladder(MP_DMP, ctrl, 2, 1) for ctrl in (3, -1)]
    want += [ladder(MP_PRODMP, CTRL_VEL, nl, 0) for nl in (1, 3, 8)]
    want += [ladder(MP_GIVEN, CTRL_POS, 5, 2), ladder(MP_NONE, 3, 3, 2)]
    want += [   # flat: the callable returns 40 + its tag; a miss returns -7, "miss", tag unset
        "flat <5, 0> v=5 -> rc=45 tag=5 calls=1 err=untouched",
        "flat <5, 0> v=0 -> rc=40 tag=0 calls=1 err=untouched",
        "flat <5, 0> v=4 -> rc=-7 tag=-99 calls=0 err=miss",
        "flat <0, 0> v=0 -> rc=40 tag=0 calls=1 err=untouched",   # a repeated value: one call
        "flat <0, 0> v=5 -> rc=-7 tag=-99 calls=0 err=miss",
        "flat <3, 7, 3, 7> v=3 -> rc=43 tag=3 calls=1 err=untouched",
        "flat <3, 7, 3, 7> v=7 -> rc=47 tag=7 calls=1 err=untouched",
        "flat <3, 7, 3, 7> v=2 -> rc=-7 tag=-99 calls=0 err=miss",
        "flat <6> v=6 -> rc=46 tag=6 calls=1 err=untouched",
        "flat <6> v=0 -> rc=-7 tag=-99 calls=0 err=miss",
    ]
    return want


@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="no hipcc")
def test_pick_reaches_each_tag_and_reports_misses(tmp_path):
    exe = str(tmp_path / "pick_table")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O1", "-std=c++17", "-Wno-unused-result",
                    os.path.join(HERE, "host", "pick_table.hip"), "-o", exe], check=True)
    got = subprocess.run([exe], check=True, capture_output=True).stdout.decode().splitlines()
    want = expected()
    assert len(want) == 48 + 10 + 10   # every hit of the ladder, its misses, the flat cases
    diff = [f"want {w!r}\n got {g!r}" for w, g in zip(want, got) if w != g]
    assert not diff and len(got) == len(want), \
        f"{len(diff)} of {len(want)} lines differ ({len(got)} printed); first:\n" + "\n".join(diff[:10])

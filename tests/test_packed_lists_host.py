"""The byte code of the packed candidate / member lists (csrc/nlk_common.h), on the CPU.

An entry is the displacement of a candidate from its target's own pixel position, (dy + r) << 4 | (dx + r) with r the
search radius the target used. nlk_host_packed_entry runs the functions the kernels themselves call: nlk_pl_word and
nlk_pl_byte (the matcher's epilogue, csrc/k_match.h), nlk_pl_decode (k_group8m's packed-list instantiation,
csrc/k_group8m.h) and nlk_pl_target_fits (the epilogue's condition for the "packed lists valid" flag). What it cannot
see is how the kernels place the bytes in the record; tests/test_packed_lists.py covers that on the GPU."""
import pytest


@pytest.mark.parametrize("r", range(1, 8))
def test_every_displacement_of_a_radius_round_trips(built, r):
    """Radii 1..7: every (dx, dy) inside the window encodes to one byte - the stated formula, all of them distinct -
    and decodes to the candidate's frame coordinate; targets away from and on the frame's border (the displacement is
    taken from the target, so a clipped window changes nothing)."""
    seen = set()
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            for px, py in ((16, 16), (0, 0), (1916, 4), (3, 1072)):
                if px + dx < 0 or py + dy < 0:
                    continue   # (no such candidate: outside the frame)
                got = built.host_packed_entry(dx, dy, r, 32, px, py)
                assert got is not None, (dx, dy, r, px, py)
                byte, back = got
                assert byte == ((dy + r) << 4 | (dx + r)) and byte < 256, (dx, dy, r, byte)
                assert back == (px + dx, py + dy), (dx, dy, r, px, py, back)
                seen.add(byte)
    assert len(seen) == (2 * r + 1) ** 2


@pytest.mark.parametrize("r", range(0, 8))
def test_a_displacement_outside_its_radius_is_refused(built, r):
    for dx, dy in ((r + 1, 0), (0, r + 1), (-r - 1, 0), (0, -r - 1), (r + 1, -r - 1)):
        assert built.host_packed_entry(dx, dy, r) is None, (dx, dy, r)


def test_radius_8_and_lists_of_33_are_refused(built):
    """What a 64-byte record cannot hold: a radius above 7 (a nibble per axis) and more than 32 candidates - the member
    list is never longer than the candidate list, so 33 members mean 33 candidates - and the smoother's pass-through
    target."""
    assert built.host_packed_entry(0, 0, 7, 32) is not None
    assert built.host_packed_entry(7, -7, 7, 32) is not None
    for dx, dy in ((0, 0), (8, 8), (-8, 3), (1, -1)):
        assert built.host_packed_entry(dx, dy, 8) is None, (dx, dy)
    assert built.host_packed_entry(0, 0, 5, 33) is None
    assert built.host_packed_entry(0, 0, 5, 2, passthrough=True) is None
    assert built.host_packed_entry(0, 0, 5, 0) is not None

"""Where linear probing puts the keys of a voxel table (sm_d_simplify.h: simp_hash, simp_probe) -- for the tests of
tests/test_register.py and tests/test_compare.py that want a probe walk to go from a table's last slot to slot 0."""


def home(key, mask):
    """simp_hash(key) & mask"""
    M = (1 << 64) - 1
    k = int(key)
    k ^= k >> 33; k = (k * 0xff51afd7ed558ccd) & M
    k ^= k >> 33; k = (k * 0xc4ceb9fe1a85ec53) & M
    return (k ^ (k >> 33)) & mask


def wraps(keys, mask):
    """keys that linear probing from simp_hash carries from the last slot of a table of mask + 1 to slot 0: how many cross that
    boundary does not depend on the insertion order"""
    used, n = set(), 0
    for k in keys:
        s = home(k, mask)
        while s in used:
            n += s == mask
            s = (s + 1) & mask
        used.add(s)
    return n


def end_run(keys, mask):
    """the keys whose home slot lies in the run of occupied slots that ends at the table's last slot.  Which keys are carried
    past the end depends on the insertion order; whichever it is, they are among these: a carried key's walk went from its home
    to the last slot over occupied slots, and which slots end up occupied does not depend on the order"""
    used = set()
    for k in keys:
        s = home(k, mask)
        while s in used:
            s = (s + 1) & mask
        used.add(s)
    first = mask + 1
    while first - 1 in used and first > 0:
        first -= 1
    return [k for k in keys if home(k, mask) >= first]

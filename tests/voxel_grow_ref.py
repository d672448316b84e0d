"""The size arithmetic of a voxel map that grows restated from the issue's definition, not from the header: the checker of
tests/test_voxel_grow_cpu.py and tests/test_voxel_grow_gpu.py."""
MAX_VOXELS = 1 << 30


def slots(max_voxels):
    """Slots of the table of a map of max_voxels voxels: the power of two >= 2 * max_voxels, at least 2."""
    return max(2, 1 << (2 * int(max_voxels) - 1).bit_length())


def ladder(m0, limit):
    """m0, min(L, 2 m0), min(L, 4 m0), ... up to the limit (limit 0, or not above m0: m0 alone)."""
    steps = [int(m0)]
    while limit > steps[-1]:
        steps.append(min(int(limit), 2 * steps[-1]))
    return steps


def capacity(m0, limit, voxels):
    """max_voxels after a call that leaves (or would leave) `voxels` voxels in a map at m0: the smallest step that holds them, else the last."""
    steps = ladder(m0, limit)
    fit = [s for s in steps if s >= voxels]
    return fit[0] if fit else steps[-1]


def capacities(m0, limit, voxels_after_calls):
    """The capacity after each of successive calls; every call starts from the capacity the one before it left."""
    out, cap = [], int(m0)
    for v in voxels_after_calls:
        cap = capacity(cap, limit, v)
        out.append(cap)
    return out

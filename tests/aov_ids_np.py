"""The matte rule of hrt_render_aov_ids_* (include/hrt.h, "id mattes and position") restated in numpy from the header's
words, sharing nothing with the HIP code: plain Python loops over pixels, samples and slots, a sort by key instead of a sorting
network, float32 scalars for the one division and the position sum.

Input: the per-sample values of every pixel, sample-major --
    object_id   [S, ...] int     the hit primitive's index, -1 for a miss
    material_id [S, ...] int     the hit's material index, -1 for a miss
    position    [S, ..., 3] f32  hitRecord::p, 0 0 0 for a miss
Output: the dict api.split_aov_ids gives -- position [..., 3], object_id [..., 4] int32, object_coverage [..., 4] float32,
material_id, material_coverage."""
import numpy as np

SLOTS = 8                    # HRT_AOV_ID_SLOTS
RANKS = 4                    # HRT_AOV_ID_RANKS
UNUSED = -2 ** 31            # the id of a rank beyond the used slots (INT32_MIN)


def table(ids):
    """One pixel, one id kind: the samples' ids in sample order -> the used slots [(id, count), ...] in slot order.  A sample whose id is
    in the table adds 1 to that slot; otherwise it takes the first empty slot; otherwise, the table full, it is dropped."""
    slots = []
    for i in ids:
        i = int(i)
        for k, (sid, n) in enumerate(slots):
            if sid == i:
                slots[k] = (sid, n + 1)
                break
        else:
            if len(slots) < SLOTS:
                slots.append((i, 1))
    return slots


def ranks(ids):
    """One pixel, one id kind -> (ids [4] int32, coverage [4] float32): the used slots by count, largest first, equal counts by id,
    smallest first (signed); the first four as id and (float)count / (float)sample_count; the rest of the four INT32_MIN and +0."""
    n = np.float32(len(ids))
    order = sorted(table(ids), key=lambda s: (-s[1], s[0]))[:RANKS]
    out_id = np.full(RANKS, UNUSED, np.int32)
    out_cov = np.zeros(RANKS, np.float32)
    for k, (sid, cnt) in enumerate(order):
        out_id[k] = sid
        out_cov[k] = np.float32(cnt) / n
    return out_id, out_cov


def mean_position(position):
    """[S, ..., 3] -> [..., 3]: the plain fp32 sum in sample order from +0, each component divided once by (float)S"""
    position = np.asarray(position, np.float32)
    total = np.zeros(position.shape[1:], np.float32)
    for s in range(position.shape[0]):
        total = total + position[s]
    return total / np.float32(position.shape[0])


def mattes(object_id, material_id, position):
    object_id, material_id = np.asarray(object_id), np.asarray(material_id)
    S, shape = object_id.shape[0], object_id.shape[1:]
    assert S >= 1 and material_id.shape == object_id.shape and np.shape(position) == object_id.shape + (3,)
    out = {"position": mean_position(position)}
    for name, ids in (("object", object_id), ("material", material_id)):
        flat = ids.reshape(S, -1)
        oid = np.empty((flat.shape[1], RANKS), np.int32)
        cov = np.empty((flat.shape[1], RANKS), np.float32)
        for i in range(flat.shape[1]):
            oid[i], cov[i] = ranks(flat[:, i])
        out[name + "_id"] = oid.reshape(shape + (RANKS,))
        out[name + "_coverage"] = cov.reshape(shape + (RANKS,))
    return out


def matte(ids, coverage, wanted):
    """[..., 4] ids and coverages -> [...]: the coverages of the ranks whose id is in `wanted`, added in rank order in fp32 from +0"""
    wanted = set(int(w) for w in np.atleast_1d(wanted))
    ids, coverage = np.asarray(ids), np.asarray(coverage, np.float32)
    out = np.zeros(ids.shape[:-1], np.float32)
    for idx in np.ndindex(*ids.shape[:-1]):
        total = np.float32(0)
        for k in range(RANKS):
            if int(ids[idx][k]) in wanted:
                total = np.float32(total + coverage[idx][k])
        out[idx] = total
    return out

"""Who computes what in the shared-prefix decode attention: a plain-Python model of the rules of include/qqq_amd_shared.h, for tests that must
know which jobs a case puts through the kernel before they trust that case.  No torch, no library: lists of Python ints in, jobs out.

The rules, as the header states them:
  root      family[i] names the first row of row i's family.  It counts only where it names a row f <= i that names itself; a row whose
            descriptor makes no sense is its own root.
  window    a family's rows fall into packs of `pack` consecutive rows counted from its first row: the window of row i starts at
            root + (i - root) // pack * pack and holds the rows of the same root among the `pack` rows from there (below b).
  joint     member j of a window takes split sp jointly iff pos[j] is in [0, max_len) and the split lies inside the first
            min(shared[j], pos[j] + 1) keys: (sp + 1) * chunk <= min(shared[j], pos[j] + 1).
  who       the first joint member of a window computes the split for all joint members.
  private   a row in range that does not take split sp jointly computes it alone up to its own pos, if the split starts at or below pos.
A row with pos outside [0, max_len) takes part in nothing."""
from collections import namedtuple

# split: index of the split; row: the batch row whose workgroup computes; base: the batch row of slot 0; live: slots (ascending), slot s
# being batch row base + s; last: the last key any live slot sees in this job
Job = namedtuple("Job", "split row base live last")


def root(family, i):
    f = family[i]
    return f if 0 <= f <= i and family[f] == f else i


def window(family, i, pack):
    """(first row, rows) of the pack window of row i"""
    r = root(family, i)
    first = r + (i - r) // pack * pack
    return first, [j for j in range(first, min(first + pack, len(family))) if root(family, j) == r]


def takes_jointly(shared, pos, j, sp, chunk, max_len):
    return 0 <= pos[j] < max_len and (sp + 1) * chunk <= min(shared[j], pos[j] + 1)


def jobs(family, shared, pos, pack, chunk, splits, max_len, G=1):
    """every job of one call, in (row, split) order.  G = h / kvh does not change who computes what; it is checked against the limit of
    64 query rows per workgroup only."""
    b = len(pos)
    assert len(family) == b and len(shared) == b and pack >= 1 and G * pack <= 64 and splits * chunk >= max_len
    out = []
    for i in range(b):
        first, rows = window(family, i, pack)
        for sp in range(splits):
            joint = [j for j in rows if takes_jointly(shared, pos, j, sp, chunk, max_len)]
            if i in joint:
                if joint[0] == i:
                    out.append(Job(sp, i, first, tuple(j - first for j in joint), (sp + 1) * chunk - 1))
            elif 0 <= pos[i] < max_len and sp * chunk <= pos[i]:
                out.append(Job(sp, i, i, (0,), min(pos[i], (sp + 1) * chunk - 1)))
    return out


def covered(job):
    """the batch rows whose partial of job.split this job writes"""
    return [job.base + s for s in job.live]


def has_hole(job):
    """a slot that is not part of the job stands below the job's last live slot: its query rows ride along as padding"""
    return len(job.live) < job.live[-1] + 1


def query_rows(job, G):
    """query rows of the workgroup up to its last live slot: slot s holds rows s * G ... s * G + G - 1 of the 16-row tiles"""
    return G * (job.live[-1] + 1)


def tiles(pack, G):
    """16-row tiles of the instantiation a call with this pack runs: one, two or four"""
    n = G * pack
    return 1 if n <= 16 else 2 if n <= 32 else 4


def straddling_slots(job, G):
    """live slots whose G rows lie in two tiles"""
    return [s for s in job.live if (s * G) // 16 != (s * G + G - 1) // 16]


def partly_shared_splits(shared, pos, chunk, splits, max_len):
    """(row, split) where the split begins inside what the row shares and ends outside it: the row must take it privately"""
    out = []
    for j in range(len(pos)):
        if 0 <= pos[j] < max_len:
            lim = min(shared[j], pos[j] + 1)
            out += [(j, sp) for sp in range(splits) if sp * chunk < lim < (sp + 1) * chunk]
    return out

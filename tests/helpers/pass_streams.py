"""Streams of searches in flight for the pass tests (pure Python; the searcher comes from the caller): the `canon` / `key`
conventions of tests/test_gpu_plane_cache.py -- whole records, cigars included -- and a stream whose steps may differ in
pattern, k and shard."""
import collections

# one search of a resident text: search_shard_begin(pattern, ptr, halo, shard_len, offset, total, k); j: what it is compared with
Job = collections.namedtuple("Job", "j pattern ptr halo shard_len offset total k")


def canon(r):
    a, pool = r.array, r.pool
    return a.tobytes(), tuple(bytes(pool[int(o):int(o) + int(l)]) for o, l in zip(a["cigar_off"], a["cigar_len"]))


def key(m):
    return (m.pattern_idx, m.text_start, m.text_end, m.pattern_start, m.pattern_end, m.cost, m.strand, m.cigar)


def whole(j, pattern, buf, n, k):
    """The job that searches all n bytes of buf."""
    return Job(j, pattern, buf.ptr, 0, n, 0, n, k)


def begin(s, job):
    return s.search_shard_begin(job.pattern, job.ptr, job.halo, job.shard_len, job.offset, job.total, job.k)


def lone(s, job):
    return s.search_shard(job.pattern, job.ptr, job.halo, job.shard_len, job.offset, job.total, job.k)


def stream(s, jobs, depth, steps, newest_first=False):
    """steps searches rotating through jobs, depth in flight: (step, job, result, stats) in finishing order"""
    out, pending = [], []
    for i in range(steps):
        job = jobs[i % len(jobs)]
        pending.append((i, job, begin(s, job)))
        if len(pending) >= depth:
            i_, job_, t = pending.pop() if newest_first else pending.pop(0)
            out.append((i_, job_, s.search_finish(t), s.stats()))
    while pending:
        i_, job_, t = pending.pop() if newest_first else pending.pop(0)
        out.append((i_, job_, s.search_finish(t), s.stats()))
    return out

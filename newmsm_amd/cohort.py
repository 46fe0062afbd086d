"""A cohort registered to one template in a single run: many pairwise registrations against one reference sphere and data, which is what the
reference's shipped pipelines do most often (gMSM_scripts/newMSM_HCP_to_template_v2.sh, run_HCP_to_template_v2.sh, gMSM_tutorial/typical_MSM.sh:
one newmsm process per subject).

Here the subjects go through a queue to worker threads of one process.  Every worker has its own Context -- and so its own stream -- and its own ops
object: no handle is ever shared between threads (the ABI's rule: calls on one handle are serialised by the caller).  What is shared is the reference
side of the feature preparation (registration.ReferenceCache: host arrays, filled by whichever worker needs a level first).  ctypes releases the GIL
inside library calls; the Python between the calls does not run in parallel (tools/time_cohort.py measures what that leaves).

Out of scope: sharing a target mesh or its direction table between contexts, and any batching of the cost kernels across subjects.
"""
import os
import queue
import threading

import numpy as np

from . import api, registration

HOST_CORES = 16  # the host set-up threads of one process (host_parallel.hpp), divided between the workers


class CohortError(RuntimeError):
    """A subject failed: the queue was stopped, the subjects that were running finished.  `subject` is its index, `results` what did finish."""

    def __init__(self, subject, cause, results):
        super().__init__("run_cohort: subject %d failed: %s: %s" % (subject, type(cause).__name__, cause))
        self.subject, self.cause, self.results = subject, cause, results


class _OwnedProductOps(registration.ProductOps):
    def close(self):
        self.ctx.close()


def product_ops(device=0, **options):
    """make_ops for the MI355X path: every call makes a ProductOps over a Context of its own (closed by run_cohort when its worker ends); `options` are
    ProductOps' own (mcmc_gpu, mcmc_draw_gpu, features_gpu), so every worker's context gets them"""
    return lambda: _OwnedProductOps(api.Context(device), **options)


def _subject_arrays(subject):
    if isinstance(subject, dict):
        return subject["xyz"], subject["tri"], subject["data"], subject.get("trans")
    return tuple(subject) + (None,) * (4 - len(subject))


def register_subject(ops, subject, ref_xyz, ref_tri, ref_data, levels, ref_cache=None, **run_kw):
    """one subject of a cohort: run_multiresolution, then transformed_data.  Returns dict(sphere_reg, level_regs, energies, labelings, transformed)"""
    xyz, tri, data, trans = _subject_arrays(subject)
    # the library takes a data matrix by its address and the mesh's vertex count: a matrix of another width would be read past its end
    if np.ndim(data) != 2 or np.shape(data)[1] != len(xyz) or np.shape(data)[0] != np.shape(ref_data)[0]:
        raise ValueError("the subject's data is %s for a sphere of %d vertices and reference data of %d rows" % (np.shape(data), len(xyz), np.shape(ref_data)[0]))
    labelings = []
    kw = dict(run_kw)
    if trans is not None:
        kw["trans_xyz"] = trans
    if ref_cache is not None:
        kw["ref_cache"] = ref_cache
    reg, level_regs, energies = registration.run_multiresolution(ops, xyz, tri, data, ref_xyz, ref_tri, ref_data, levels, labelings_out=labelings, **kw)
    moved, target = ops.mesh(reg, tri), ops.mesh(ref_xyz, ref_tri)
    transformed = registration.transformed_data(ops, moved, data, target, ref_data, excl=run_kw.get("excl", False), cutthr=run_kw.get("cutthr", (0.0, 0.0001)),
                                                intensity=run_kw.get("intensity", False))
    return dict(sphere_reg=reg, level_regs=level_regs, energies=energies, labelings=labelings, transformed=np.array(transformed))


def run_cohort(make_ops, subjects, ref_xyz, ref_tri, ref_data, levels, workers=1, ref_cache=None, **run_kw):
    """Registers every subject to the one reference.

    make_ops   called once in every worker thread: the worker's own ops object (product_ops(): a ProductOps over a Context of its own).  An ops
               object with a close() gets it called when its worker ends.
    subjects   per subject (xyz, tri, data[, trans_xyz]) or dict(xyz=, tri=, data=[, trans=]): its input sphere (radius 100), its D x V data and,
               optionally, its sphere.reg of an earlier run (--trans)
    ref_*      the reference sphere and data; levels, run_kw: as run_multiresolution takes them
    workers    threads that take subjects from the queue, at most one per subject
    ref_cache  a registration.ReferenceCache to use (and fill); a fresh one by default

    Returns the subjects' results (register_subject) in subject order, whatever the order of completion.  A subject that raises -- a HIP error
    reported by the library included -- stops the queue: subjects that are running finish, nothing further starts, CohortError names the subject
    (the lowest index when several failed).  The host set-up threads are divided between the workers: MSMHIP_HOST_THREADS = max(1, 16 // workers)
    for the length of the run unless the caller's environment sets it (the library reads it per call); no other variable is touched."""
    subjects = list(subjects)
    S = len(subjects)
    workers = max(1, min(int(workers), S)) if S else 1
    cache = ref_cache if ref_cache is not None else registration.ReferenceCache()
    todo = queue.Queue()
    for s in range(S):
        todo.put(s)
    results, errors = [None] * S, {}
    stop = threading.Event()

    def work():
        ops = None
        try:
            ops = make_ops()
        except Exception as e:  # noqa: BLE001 -- reported against the subject this worker would have taken
            try:
                errors[todo.get_nowait()] = e
            except queue.Empty:
                pass
            stop.set()
            return
        try:
            while not stop.is_set():
                try:
                    s = todo.get_nowait()
                except queue.Empty:
                    return
                try:
                    results[s] = register_subject(ops, subjects[s], ref_xyz, ref_tri, ref_data, levels, ref_cache=cache, **run_kw)
                except Exception as e:  # noqa: BLE001
                    errors[s] = e
                    stop.set()
        finally:
            close = getattr(ops, "close", None)
            if close is not None:
                close()

    ours = "MSMHIP_HOST_THREADS" not in os.environ
    if ours:
        os.environ["MSMHIP_HOST_THREADS"] = str(max(1, HOST_CORES // workers))
    try:
        if workers == 1:
            work()  # on the caller's thread: nothing to hand over
        else:
            threads = [threading.Thread(target=work, name="cohort-%d" % k) for k in range(workers)]
            for t in threads:
                t.start()
            for t in threads:
                t.join()
    finally:
        if ours:
            del os.environ["MSMHIP_HOST_THREADS"]
    if errors:
        first = min(errors)
        raise CohortError(first, errors[first], results) from errors[first]
    return results

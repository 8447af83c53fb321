"""What the tools/*_batch_probe.py share: the command line, the collected lines and their --out file, the library that route (a) runs on, the
timing of one enqueued pass of route (b), alternating passes, a kernel's own time through the profile drain, the bitwise comparison of floats, the closing JSON
line and the exit status.  A probe keeps what is its own: the workload,
the loop (a), the call (b) and the comparison of their results."""
import argparse, ctypes as C, json, sys, time
import numpy as np
import torch


def med(v):
    return float(np.median(v))


def big_vocab(rng, k=10, L=6):
    """a full k-ary tree of L levels in DBoW2's numbering, level by level: (L, child_ptr, children, node_desc, word_id, weight)"""
    sizes = [k ** l for l in range(L + 1)]
    offs = np.concatenate([[0], np.cumsum(sizes)])
    n = int(offs[-1])
    desc = np.zeros((n, 32), np.uint8)
    desc[0] = rng.integers(0, 256, 32, dtype=np.uint8)
    for l in range(1, L + 1):
        par = np.repeat(desc[offs[l - 1]:offs[l]], k, axis=0)
        flips = rng.integers(0, 256, par.shape, dtype=np.uint8)
        for _ in range(min(l - 1, 2)):                      # flip probability 1/2, 1/4, 1/8, 1/8, ..: children cluster around their parent
            flips &= rng.integers(0, 256, par.shape, dtype=np.uint8)
        desc[offs[l]:offs[l + 1]] = par ^ flips
    nchild = np.zeros(n, np.int64); nchild[:offs[L]] = k
    ptr = np.concatenate([[0], np.cumsum(nchild)]).astype(np.int32)
    children = np.arange(1, n, dtype=np.int32)
    word = np.full(n, -1, np.int32); word[offs[L]:] = np.arange(sizes[L], dtype=np.int32)
    weight = np.zeros(n, np.float64); weight[offs[L]:] = rng.uniform(0.1, 9.0, sizes[L])
    return L, ptr, children, desc, word, weight


def parse_args(sizes_flag, sizes, reps, unique, loop_lib=True):
    """--batches or --sessions (a.sizes: the list of ints), --reps, --unique, --out, and --loop-lib where route (a) may run on another library"""
    ap = argparse.ArgumentParser()
    ap.add_argument(sizes_flag, dest="sizes", default=sizes); ap.add_argument("--reps", type=int, default=reps); ap.add_argument("--unique", type=int, default=unique)
    if loop_lib: ap.add_argument("--loop-lib", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    a.sizes = [int(x) for x in a.sizes.split(",")]
    return a


class Lines:
    """say(s) prints a line and keeps it; finish() adds the JSON line, writes --out and ends the process non-zero where (b) differed from (a)"""
    def __init__(self):
        self.lines = []

    def say(self, s):
        print(s, flush=True); self.lines.append(s)

    def finish(self, name, report, out, equal=True):
        self.say("JSON " + json.dumps(report))
        if out:
            with open(out, "w") as f:
                f.write("\n".join(self.lines) + "\n")
        if not equal:
            print("%s: (b) differs from (a)" % name, file=sys.stderr)
            sys.exit(1)


def loop_library(fe, ctx, a, say):
    """-> (library, context handle) of route (a): --loop-lib with a context of its own, else the library under test and ctx"""
    LA = C.CDLL(a.loop_lib) if a.loop_lib else fe.lib()
    LA.sslam_last_error.restype = C.c_char_p
    hA = C.c_void_p()
    if a.loop_lib:
        assert LA.sslam_ctx_create(0, C.byref(hA)) == 0
    else:
        hA = ctx.h
    say("(a) runs on %s" % (a.loop_lib or "the library under test"))
    return LA, hA


def timed_pass(st, enqueue):
    """one pass of (b) on the side stream st -> (device ms between two events, wall ms to the end of the stream synchronise, ms spent enqueueing)"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record(st)
    enqueue()
    t1 = time.perf_counter()
    e1.record(st); st.synchronize()
    return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3, (t1 - t0) * 1e3


def alternate(reps, run_a, run_b):
    """reps alternating passes -> (every result of run_a, every result of run_b)"""
    ta, tb = [], []
    for _ in range(reps):
        ta.append(run_a()); tb.append(run_b())
    return ta, tb


def b_medians(tb):
    """-> the medians of (device ms, wall ms, enqueue ms) over the passes of timed_pass"""
    return tuple(med([x[i] for x in tb]) for i in range(3))


def drain(L, h):
    """sslam_profile_drain of context h on library L -> {kernel name: ms} since the last drain"""
    names = (C.c_char_p * 16)(); ms = (C.c_double * 16)(); cnt = (C.c_int * 16)()
    n = L.sslam_profile_drain(h, names, ms, cnt, 16)
    return {names[i].decode(): ms[i] for i in range(n)}


def kernel_passes(L, h, st, enqueue, kernel, reps):
    """a kernel's own time: a warm-up pass and `reps` passes of enqueue() on stream st with the profile on -> the ms of `kernel` in each of the `reps`"""
    L.sslam_profile_enable(h, 1)
    k = []
    for _ in range(reps + 1):
        enqueue(); st.synchronize()
        k.append(drain(L, h)[kernel])
    L.sslam_profile_enable(h, 0)
    return k[1:]


def same_floats(a, b):
    """float32 values alike bit for bit, a NaN equal to any NaN"""
    return bool(((np.ascontiguousarray(a, np.float32).view(np.uint32) == np.ascontiguousarray(b, np.float32).view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())

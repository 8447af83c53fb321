"""What the host models of the RANSAC units share (tests/two_view_sim.py, tests/sim3_sim.py): a stand-alone program under tests/sim/ that compiles a csrc/*_math.h header
with plain g++, built once with -O2 -ffp-contract=off and once more under -fsanitize=address,undefined -- both once per process and source, whichever module asks first;
nothing is loaded into Python.  run(src, text) sends the text through both builds: both must exit 0 with an empty stderr and answer alike.  bits / ints write float32
bit patterns and integers as the programs read them, floats reads bit patterns back."""
import atexit, functools, os, shutil, subprocess, tempfile
import numpy as np


@functools.lru_cache(maxsize=None)
def programs(src, defines=()):
    """(plain, sanitised): the two builds of the sim, in a directory that goes away with the process; defines: -D options of a build variant (a tuple of NAME=value)"""
    name = os.path.splitext(os.path.basename(src))[0]
    d = tempfile.mkdtemp(prefix=name + "_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    plain, san = os.path.join(d, name), os.path.join(d, name + "_san")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", src, "-o", plain] + ["-D" + d for d in defines])
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", san] + ["-D" + d for d in defines])
    return plain, san


def bits(a):
    return " ".join(map(str, np.ascontiguousarray(a, np.float32).view(np.uint32).ravel().tolist()))


def ints(a):
    return " ".join(map(str, np.asarray(a, np.int64).ravel().tolist()))


def floats(tokens):
    return np.array([int(t) for t in tokens], np.uint64).astype(np.uint32).view(np.float32)


def run_plain(src, text, defines=()):
    """the plain build alone -> its stdout"""
    r = subprocess.run([programs(src, tuple(defines))[0]], input=text, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    return r.stdout


def run(src, text):
    """both builds -> the stdout they share"""
    outs = []
    for exe in programs(src):
        r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and r.stderr == "", (exe, r.returncode, r.stderr[-2000:])
        outs.append(r.stdout)
    assert outs[0] == outs[1], "the plain and the sanitised build of the sim answer differently"
    return outs[0]

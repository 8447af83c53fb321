"""The plans of csrc/match_plan.h and the form plan of csrc/lines_form.h as the test modules ask for them.  The headers hold no HIP: a dump program under tests/sim/
(match_plan_dump.cpp unless the caller names another, e.g. LINES_FORM) compiles one with plain g++, once as it is and once with -fsanitize=address,undefined, as a
stand-alone program -- both once per process and source, whichever module asks first; nothing is loaded into Python.  asker(family) returns ask(lines) -> one list of
tokens per line for the lines of that family (proj_batch, bow_batch, tri_batch, fuse_batch, distinct_batch; None: the un-prefixed commands).  Every call runs both
builds: both must exit 0 with an empty stderr and answer alike, one row per line."""
import atexit, functools, os, shutil, subprocess, tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "sim", "match_plan_dump.cpp")
LINES_FORM = os.path.join(HERE, "sim", "lines_form_dump.cpp")


@functools.lru_cache(maxsize=None)
def programs(src=SRC):
    """(plain, sanitised): the two builds of the dump program `src`, in a directory that goes away with the process"""
    name = os.path.splitext(os.path.basename(src))[0]
    d = tempfile.mkdtemp(prefix=name + "_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    plain, san = os.path.join(d, name), os.path.join(d, name + "_san")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", src, "-o", plain])
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", san])
    return plain, san


def asker(family=None, src=SRC):
    prefix = family + " " if family else ""

    def ask(lines):
        text = "".join(prefix + l + "\n" for l in lines)
        outs = []
        for exe in programs(src):
            r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
            assert r.returncode == 0 and r.stderr == "", (exe, r.returncode, r.stderr)
            outs.append(r.stdout)
        assert outs[0] == outs[1]
        rows = [l.split() for l in outs[0].splitlines()]
        assert len(rows) == len(lines)
        return rows
    return ask

"""A fork()ed child of a process that uses the library must never finalize the parent's device objects (the HIP runtime does not
survive a fork): _lib registers gc.freeze() to run in the child, so everything inherited sits in the permanent generation there and
the child's collector sees only what the child itself creates.  No GPU: a cycle with a finalizer stands in for a device object."""
import gc
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from aozora_sdxl_training_amd import _lib      # noqa: E402,F401   (registers the hook)


class _Device:
    """Stands in for a device object in a reference cycle; its finalizer reports the process it ran in."""
    def __init__(self, fd):
        self.fd, self.me = fd, self

    def __del__(self):
        os.write(self.fd, b"finalized in %d\n" % os.getpid())


def test_forked_child_freezes_inherited_objects_and_runs_none_of_their_finalizers():
    r, w = os.pipe()
    gc.collect()
    assert gc.get_freeze_count() == 0
    gc.disable()                       # the garbage must still be there at the fork
    try:
        _Device(w)                     # cyclic garbage, uncollected
        pid = os.fork()
        if pid == 0:                   # the child: collect, report, leave without running the interpreter's exit path
            code = 1
            try:
                frozen = gc.get_freeze_count()
                gc.enable()
                gc.collect()
                os.write(w, b"child frozen %d\n" % frozen)
                code = 0
            finally:
                os._exit(code)
        _, status = os.waitpid(pid, 0)
    finally:
        gc.enable()
    assert status == 0
    gc.collect()                       # the parent finalizes its own object
    os.close(w)
    out = os.read(r, 4096).decode().splitlines()
    os.close(r)
    assert out[0].startswith("child frozen ") and int(out[0].split()[-1]) > 0, out
    assert out[1:] == [f"finalized in {os.getpid()}"], out
    assert gc.get_freeze_count() == 0          # the parent itself is not frozen

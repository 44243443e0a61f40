"""CPU: every ctypes prototype of _lib.py takes as many arguments as include/unet_hip.h declares.  A prototype one argument short still loads and runs:
ctypes passes the surplus argument as a C int, so a trailing pointer (the stream) reaches the library with its upper 32 bits undefined."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_binding_has_the_declared_argument_count():
    from covidseg_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "unet_hip.h")).read()
    hdr = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    seen = {}
    for m in re.finditer(r"\b(unet_[a-zA-Z0-9_]+)\s*\(([^;{]*?)\)\s*;", hdr):
        params = m.group(2).strip()
        seen[m.group(1)] = 0 if params in ("", "void") else params.count(",") + 1
    wrong = {name: (seen[name], len(args)) for name, (_, args) in _lib._PROTOS.items() if name in seen and seen[name] != len(args)}
    assert not wrong, f"(declared, bound) argument counts differ: {wrong}"
    assert "unet_gather_samples" in seen and "unet_augment_samples" in seen

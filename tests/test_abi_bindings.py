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
    assert "unet_conv3x3_fwd_ld" in seen and "unet_conv3x3_fwd_ld" in _lib._PROTOS
    assert "unet_conv3x3_bnfold_bwd_data" in seen and "unet_conv3x3_bnfold_bwd_data" in _lib._PROTOS


def test_every_bf16_entry_is_called_by_a_gpu_test():
    """every _bf16 entry point of include/unet_hip.h is called (lib.<name>() by some tests/test_gpu_*.py: a bf16 instance that no per-op test calls is only seen
    through the model tests, whose bounds are far looser than one kernel's rounding"""
    hdr = open(os.path.join(ROOT, "include", "unet_hip.h")).read()
    hdr = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    names = sorted(set(re.findall(r"\b(unet_\w*_bf16\w*)\s*\(", hdr)))
    assert len(names) >= 17
    tests = os.path.join(ROOT, "tests")
    src = "".join(open(os.path.join(tests, f)).read() for f in sorted(os.listdir(tests)) if f.startswith("test_gpu_") and f.endswith(".py"))
    missing = [n for n in names if f"lib.{n}(" not in src]
    assert not missing, f"bf16 entries no GPU test calls: {missing}"

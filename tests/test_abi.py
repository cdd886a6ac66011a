"""CPU-side checks of the drop-in boundary: the C-ABI library is present, loads, and exports
exactly the entry points include/badger_pf.h declares (no compute call is made here)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "badger_pf.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(bpf_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    from badger_amcl_amd import build
    so = build.build()
    lib = ctypes.CDLL(so)
    names = declared_symbols()
    assert len(names) >= 40
    for n in names:
        assert hasattr(lib, n), "missing export " + n


def test_python_binding_covers_the_header():
    from badger_amcl_amd import _lib
    assert sorted(_lib.SIGNATURES) == declared_symbols()
    _lib.load()


def test_no_gpu_fails_loudly_not_silently():
    """Without a GPU bpf_create must return an error; with one it must succeed.  Either way the
    package never computes on the CPU."""
    import badger_amcl_amd as bpf
    try:
        import torch
        has_gpu = torch.cuda.is_available()
    except Exception:
        has_gpu = False
    if has_gpu:
        e = bpf.Engine(0)
        e.close()
    else:
        with pytest.raises(bpf.BpfError):
            bpf.Engine(0)


def test_product_code_never_touches_the_oracle():
    pkg = os.path.join(ROOT, "badger_amcl_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".inl", ".h", ".cpp")):
                text = open(os.path.join(dirpath, f), errors="ignore").read()
                assert "pyoracle" not in text and "amcl_oracle" not in text, f
                assert not re.search(r"^\s*(from|import)\s+oracle\b", text, flags=re.M), f


CSRC = os.path.join(ROOT, "badger_amcl_amd", "csrc")
COPY_HOME = "host_copy.hpp"
# the functions of host_copy.hpp that may take a plain (void*) host address: the pageable ways up and down, which
# decide between the bounce buffer and the runtime ...
PAGEABLE_COPIES = {"h2d_from_host", "h2d_from_host_sync", "d2h_to_host"}
# ... and the two that only look an address up among the registered ranges and never copy
ADDRESS_LOOKUPS = {"host_reg_find", "host_direct_ok"}


def code_of(path):
    """A C++ source without its comments (the prose may name the runtime's calls; code may not)."""
    text = open(path, errors="ignore").read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def test_copies_live_in_one_file():
    """Every hipMemcpy* of csrc/ is in host_copy.hpp.  The walk takes every file, collectives_rccl.cpp (a separate
    library that copies nothing) included.  One exception by name: hipMemcpyFromSymbol in the BPF_PHASE_TIMING
    diagnostic build reads a device symbol of at most 512 KB into the tool's buffer and has no engine to bounce
    through; the product build does not compile it."""
    users = {}
    for f in sorted(os.listdir(CSRC)):
        found = set(re.findall(r"\bhipMemcpy\w*", code_of(os.path.join(CSRC, f))))
        kinds = {"hipMemcpyHostToDevice", "hipMemcpyDeviceToHost", "hipMemcpyDeviceToDevice", "hipMemcpyDefault",
                 "hipMemcpyHostToHost", "hipMemcpyKind"}
        calls = found - kinds
        if f != COPY_HOME:
            assert not (found & kinds), (f, found & kinds)
            calls -= {"hipMemcpyFromSymbol"}
        if calls:
            users[f] = calls
    assert users == {COPY_HOME: {"hipMemcpyAsync"}}, users


def test_only_the_pageable_copies_take_a_plain_host_address():
    text = code_of(os.path.join(CSRC, COPY_HOME))
    # a definition in this code's style: name(parameters) and the opening brace alone in column 0, body to the next
    # closing brace in column 0
    functions = re.findall(r"\b(\w+)\s*\(([^()]*)\)\s*\n\{\n(.*?)\n\}\n", text, flags=re.S)
    names = [name for name, _, _ in functions]
    assert PAGEABLE_COPIES | ADDRESS_LOOKUPS | {"pinned_up", "pinned_down", "small_down", "copy_d2d"} <= set(names)
    assert len(names) == len(set(names)), names
    copying = set()
    for name, params, body in functions:
        takes_void = re.search(r"\bvoid\s*\*", params) is not None
        assert takes_void == (name in PAGEABLE_COPIES | ADDRESS_LOOKUPS), name
        if "hipMemcpy" not in body:
            continue
        copying.add(name)
        assert name not in ADDRESS_LOOKUPS
        if name in PAGEABLE_COPIES:
            continue
        if name == "copy_d2d":
            assert set(re.findall(r"\bhipMemcpy[A-Z]\w*To\w*", body)) == {"hipMemcpyDeviceToDevice"}
        elif name == "small_down":  # the host side is the engine's pinned scratch
            assert re.search(r"hipMemcpyAsync\(e->h_small\.p \+ at,", body), body
        else:                       # the host side is a PinnedBuf, passed as the buffer
            assert "PinnedBuf<" in params, name
            ends = r"(dev\.p \+ dev_off, host\.p \+ host_off|host\.p \+ host_off, dev\.p \+ dev_off)"
            assert re.search(r"hipMemcpyAsync\(" + ends + ",", body), body
    assert copying == {"h2d_from_host", "d2h_to_host", "pinned_up", "pinned_down", "small_down", "copy_d2d"}

"""The signature tables of the four pass-handle modules against the built library and include/jsmpeg_hip.h: every name of a
table is exported and bound as the table says, and the tables name exactly the functions their part of the header declares.
No device is needed: the library is loaded, nothing is called."""
import importlib
import os
import re

import pytest

from conftest import ROOT

#          module, what its part's functions are called in the header
PARTS = [("resample", r"resample(?:r_)?"), ("logmel", r"logmel_"), ("mp2_encode", r"mp2_encoder_"), ("ts_program", r"ts_program_")]


@pytest.mark.parametrize("name,prefix", PARTS, ids=[p[0] for p in PARTS])
def test_the_table_is_the_binding_and_the_header(name, prefix, hip_lib):
    mod = importlib.import_module("jsmpeg_amd." + name)
    table = mod.SIGNATURES
    assert mod.SYMBOLS == tuple(table) and len(set(mod.SYMBOLS)) == len(mod.SYMBOLS)
    L = mod.lib()
    for symbol, (restype, argtypes) in table.items():
        fn = getattr(L, symbol)                                   # AttributeError: the library does not export it
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), symbol
    with open(os.path.join(ROOT, "include", "jsmpeg_hip.h")) as f:
        declared = set(re.findall(r"\b(jsmpeg_hip_%s\w*)\(" % prefix, f.read()))
    assert declared == set(table)


def test_device_read_is_bound_once(hip_lib):
    from jsmpeg_amd import _pass, logmel, mp2_encode, resample, ts_program
    L = _pass.lib()
    assert all(m.lib() is L for m in (resample, logmel, mp2_encode, ts_program))
    assert L.jsmpeg_hip_device_read.restype is _pass.c_int and L.jsmpeg_hip_device_read.argtypes == [_pass.vp, _pass.vp, _pass.u64]
    assert not any("jsmpeg_hip_device_read" in m.SIGNATURES for m in (resample, logmel, mp2_encode, ts_program))

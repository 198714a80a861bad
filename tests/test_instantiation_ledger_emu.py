"""CPU-only: every kernel instantiation the library compiles has a row in tests/instantiation_cases.py, and that row, run on
tests/hipemu's lockstep emulation, launches exactly that instantiation (the emulator's launch log) and passes its check.

  (a) the compiled set: `nm -C` on libfcd_emu.so -- csrc/*.hip compiled unchanged, and the launch macro takes every
      kernel's address, so each instantiation the sources launch has a symbol there;
  (b) the same set read off the gfx950 code objects in libfcd_hip.so (where objcopy and the ROCm LLVM tools exist);
  (c) compiled == the ledger's rows + its exemptions (a newly compiled instantiation without a row fails there, and so
      does a row nothing compiles), and one test per row.
The exemptions (instantiation_cases.EXEMPT) are kernels no entry point of include/fcd.h reaches in a default build."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import pytest

import instantiation_cases as IC
from emu_util import emu_lib_path, emulated_kernels

LLVM = "/opt/rocm/lib/llvm/bin"


def _kernel_names(demangled_lines):
    out = set()
    for line in demangled_lines:
        if "kname<" in line or "lambda" in line or "hipemu::launch" in line:
            continue
        c = IC.canonical(line)
        if re.match(r"^\w+_kernel(<.*>)?$", c):
            out.add(c)
    return out


def compiled_emu():
    txt = subprocess.check_output(["nm", "-C", "--defined-only", emu_lib_path()]).decode()
    lines = [l.split(" ", 2)[2] for l in txt.splitlines() if re.match(r"^[0-9a-f]+ [tTwW] ", l)]
    return _kernel_names(l for l in lines if "(" in l)  # (a C++ signature: not the extern "C" entry points)


ROWS = {name: (case, args) for name, case, args in IC.rows()}
EXEMPT = {name: why for name, why in IC.EXEMPT}


@pytest.fixture(scope="module")
def compiled():
    return compiled_emu()


@pytest.fixture(scope="module")
def fcd():
    import fast_ctc_decode_amd as m
    with emulated_kernels() as lib:
        lib.hipemu_launch_log_read.restype = C.c_size_t
        lib.hipemu_launch_log_read.argtypes = [C.c_char_p, C.c_size_t]
        yield m, lib


def launched(lib):
    need = lib.hipemu_launch_log_read(None, 0)
    buf = C.create_string_buffer(need)
    assert lib.hipemu_launch_log_read(buf, need) == need
    return {IC.canonical(l) for l in buf.value.decode().splitlines() if l}


def test_device_build_compiles_the_same_instantiations(compiled):
    """(b): the kernel symbols of every gfx950 code object in libfcd_hip.so, demangled"""
    cxxfilt = LLVM + "/llvm-cxxfilt" if os.path.exists(LLVM + "/llvm-cxxfilt") else shutil.which("c++filt")
    tools = [shutil.which("objcopy"), LLVM + "/clang-offload-bundler", LLVM + "/llvm-readelf", cxxfilt]
    if not all(t and os.path.exists(t) for t in tools):
        pytest.skip("objcopy / the ROCm LLVM tools / a demangler are not installed")
    from fast_ctc_decode_amd import _native, build
    build.build()
    tmp = tempfile.mkdtemp(prefix="fcd_ledger_")
    mangled = set()
    try:
        subprocess.check_call(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", _native.LIB_PATH, tmp + "/fat.bin"])
        blob = open(tmp + "/fat.bin", "rb").read()
        starts = [m.start() for m in re.finditer(re.escape(b"__CLANG_OFFLOAD_BUNDLE__"), blob)] + [len(blob)]
        for a, b in zip(starts, starts[1:]):
            with open(tmp + "/one.bin", "wb") as f:
                f.write(blob[a:b])
            subprocess.check_call([LLVM + "/clang-offload-bundler", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                                   "--input=" + tmp + "/one.bin", "--output=" + tmp + "/dev.co", "--unbundle"])
            if os.path.getsize(tmp + "/dev.co") == 0:
                continue  # (a translation unit without device code)
            notes = subprocess.check_output([LLVM + "/llvm-readelf", "--notes", tmp + "/dev.co"]).decode()
            mangled |= set(re.findall(r"\.name:\s+(\S+)", notes))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    mangled = sorted(m for m in mangled if m.startswith("_Z"))
    demangled = subprocess.check_output([cxxfilt], input="\n".join(mangled).encode()).decode().splitlines()
    device = _kernel_names(demangled)
    assert device == compiled, (sorted(device - compiled), sorted(compiled - device))


def test_every_compiled_instantiation_has_a_row(compiled):
    """(c), first half: compiled == rows + exemptions, in both directions"""
    missing = sorted(compiled - set(ROWS) - set(EXEMPT))
    assert not missing, "compiled, and no row in tests/instantiation_cases.py: %s" % missing
    assert not (set(ROWS) - compiled), "rows nothing compiles: %s" % sorted(set(ROWS) - compiled)
    assert not (set(EXEMPT) & set(ROWS))
    assert not (set(EXEMPT) - compiled), "an exemption for a kernel that no longer exists"
    assert all(why.strip() for why in EXEMPT.values())


def test_every_kernel_is_named_as_the_compiled_sets_expect():
    """both compiled sets are read off symbols named *_kernel: every __global__ function under csrc/ is named so (a kernel
    of another name would be invisible to (a), (b) and (c))"""
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fast_ctc_decode_amd", "csrc")
    found = []
    for f in sorted(os.listdir(csrc)):
        if f.endswith((".hip", ".h", ".inc")):
            text = re.sub(r"//[^\n]*", "", open(os.path.join(csrc, f)).read())
            # (`__global__ [__launch_bounds__(...)] [__attribute__((...))] void name(` on one line)
            found += [(f, m) for m in re.findall(r"__global__\b.*?\bvoid\s+(\w+)\s*\(", text)]
            assert len(re.findall(r"__global__", text)) == sum(1 for g, _ in found if g == f), (f, "a __global__ this test cannot read")
    assert len(found) >= 37, found
    assert all(name.endswith("_kernel") for _, name in found), [x for x in found if not x[1].endswith("_kernel")]


@pytest.mark.parametrize("name", sorted(ROWS))
def test_instantiation(fcd, name, monkeypatch):
    m, lib = fcd
    seen = set()

    def probe():  # the names launched since the last look; the beam rows look around every call they make
        got = launched(lib)
        lib.hipemu_launch_log_reset()
        seen.update(got)
        return got
    monkeypatch.setattr(IC, "PROBE", probe)
    lib.hipemu_launch_log_reset()
    IC.run(m, name)
    probe()
    template = IC.parse(name)[0]
    same = {n for n in seen if IC.parse(n)[0] == template}
    assert same == {name}, "the row launched %s" % sorted(same)

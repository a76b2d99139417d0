"""Does the HIP runtime here import, in a second process, the fd a first process exported from a
hipMemCreate chunk?  That is how snapshot slots of 1.5 GiB and more (or any with DPWA_VMM=1) reach
the peers.  The runtime is asked directly, through ctypes on the libamdhip64 a torch process holds
(the one libdpwa_hip.so runs on): nothing of dpwa_amd is loaded, so a fault of the project's own
import path cannot look like a machine without the facility.

Run without arguments: the exporter creates one chunk, exports it and starts this file again as
the importer (which inherits the fd).  The importer hands the fd over as its runtime takes it:
by value, then through a pointer, from HIP 7.2 on; through a pointer only before (7.0 reads
*osHandle and takes a segmentation fault on an fd passed as the pointer value,
tools/vmm_torch_probe.py).  Exit status 0: imported; 3: hipErrorInvalidValue under every form tried
(the forms and the runtime's version on stdout); anything else: something else went wrong.
tests/helpers.py need_fd_sharing asks this once per session."""
import ctypes
import os
import subprocess
import sys


class Loc(ctypes.Structure):
    _fields_ = [("type", ctypes.c_int), ("id", ctypes.c_int)]


class Flags(ctypes.Structure):
    _fields_ = [("compressionType", ctypes.c_ubyte), ("gpuDirectRDMACapable", ctypes.c_ubyte),
                ("usage", ctypes.c_ushort)]


class Prop(ctypes.Structure):           # hipMemAllocationProp
    _fields_ = [("type", ctypes.c_int), ("requestedHandleType", ctypes.c_int), ("location", Loc),
                ("win32HandleMetaData", ctypes.c_void_p), ("allocFlags", Flags)]


PINNED, POSIX_FD, DEVICE, INVALID_VALUE = 1, 1, 1, 1


def runtime():
    """The libamdhip64 of a torch process, and its version."""
    import torch
    torch.cuda.init()
    path = "libamdhip64.so.7"           # the soname of torch's bundled runtime: the loaded one answers
    try:
        with open("/proc/self/maps") as f:
            path = sorted({ln.split()[-1] for ln in f if "libamdhip64" in ln})[0]
    except (OSError, IndexError):
        pass
    lib = ctypes.CDLL(path)
    lib.hipGetErrorString.restype = ctypes.c_char_p
    check(lib, lib.hipSetDevice(0), "hipSetDevice")
    v = ctypes.c_int()
    check(lib, lib.hipRuntimeGetVersion(ctypes.byref(v)), "hipRuntimeGetVersion")
    return lib, v.value


def check(lib, rc, what):
    if rc:
        raise RuntimeError("%s: %s" % (what, lib.hipGetErrorString(rc).decode()))


def importer(fd):
    lib, version = runtime()
    forms = ["value", "pointer"] if version >= 70200000 else ["pointer"]
    for form in forms:
        h, by_ptr = ctypes.c_ulonglong(), ctypes.c_int(fd)
        rc = lib.hipMemImportFromShareableHandle(ctypes.byref(h), ctypes.c_void_p(fd) if form == "value"
                                                 else ctypes.byref(by_ptr), POSIX_FD)
        if rc == 0:
            check(lib, lib.hipMemRelease(h), "hipMemRelease")
            return 0
        if rc != INVALID_VALUE:
            raise RuntimeError("hipMemImportFromShareableHandle (fd by %s): %s"
                               % (form, lib.hipGetErrorString(rc).decode()))
    print("HIP runtime %d: hipMemImportFromShareableHandle of another process's fd, passed by %s: invalid argument"
          % (version, " and by ".join(forms)))
    return 3


def exporter():
    lib, _ = runtime()
    prop = Prop(PINNED, POSIX_FD, Loc(DEVICE, 0), None, Flags(0, 0, 0))
    gran = ctypes.c_size_t()
    check(lib, lib.hipMemGetAllocationGranularity(ctypes.byref(gran), ctypes.byref(prop), 1), "granularity")
    unit = max(gran.value, 2 << 20)
    size = (2 << 20) + unit - 1
    size -= size % unit
    h, fd = ctypes.c_ulonglong(), ctypes.c_int(-1)
    check(lib, lib.hipMemCreate(ctypes.byref(h), ctypes.c_size_t(size), ctypes.byref(prop), ctypes.c_ulonglong(0)),
          "hipMemCreate")
    check(lib, lib.hipMemExportToShareableHandle(ctypes.byref(fd), h, POSIX_FD, ctypes.c_ulonglong(0)),
          "hipMemExportToShareableHandle")
    rc = subprocess.run([sys.executable, os.path.abspath(__file__), str(fd.value)], pass_fds=[fd.value],
                        timeout=60).returncode
    os.close(fd.value)
    check(lib, lib.hipMemRelease(h), "hipMemRelease")
    return rc


if __name__ == "__main__":
    sys.exit(importer(int(sys.argv[1])) if len(sys.argv) > 1 else exporter())

"""Which kernel form an entry point launches for a shape, asked of the library: `ptr_launch_form` (include/ptranking_amd.h lists each entry
point's arguments and form values) calls the function the entry point's own launcher calls.  No GPU is needed; the PTR_* switches are read
per call, so a test sets them with monkeypatch."""
import ctypes

N_FORM = 8


def launch_form(entry, *args):
    """The form values of `entry` for `args`, as a tuple of N_FORM ints (zeros beyond the entry's own count)."""
    from ptranking_amd import _lib
    lib = _lib.load()
    a = (ctypes.c_int64 * max(1, len(args)))(*[int(v) for v in args])
    out = (ctypes.c_int32 * N_FORM)()
    rc = lib.ptr_launch_form(entry.encode(), a, len(args), out, N_FORM)
    assert rc == 0, (entry, args, lib.ptr_last_error())
    return tuple(out)


def group_form(entry, *args):
    """(G, DPT) or (G, TP) of the entry points whose form is just that pair: threads per query, documents per thread or subtopic tile."""
    return launch_form(entry, *args)[:2]


def ring_or_tiling(entry, L):
    """("ring", DPT) or ("lds", G, DPT) of the smooth-rank entry points."""
    ring, g, dpt = launch_form(entry, L)[:3]
    return ("ring", dpt) if ring else ("lds", g, dpt)

"""``LaunchList``: the C-ABI launches a plan lists once per batch geometry and replays from Python.  ``add`` converts an argument
and keeps what it points at in the same step, ``run`` is the one replay loop.  (HRNet's ``Engine`` replays native programs instead.)"""
import ctypes as C

import torch

from . import capi


class LaunchList:
    def __init__(self, keep=None):
        self.calls = []                            # (fn, name, args): args without the stream, in the form ctypes takes
        self.keep = [] if keep is None else keep   # the lists of one plan may share it

    def add(self, name: str, *args) -> None:
        """List ``name(*args, stream)``.  A tensor goes as its data pointer, a ctypes structure by reference (the very object: a field
        set later is seen by the next run); both are kept.  The rest passes as it is: the owner behind a raw address is the caller's."""
        conv = []
        for a in args:
            if isinstance(a, (torch.Tensor, C.Structure)):
                self.keep.append(a)
                a = C.c_void_p(a.data_ptr()) if isinstance(a, torch.Tensor) else C.byref(a)
            conv.append(a)
        self.calls.append((getattr(capi.lib(), name), name, tuple(conv)))

    def keep_alive(self, *objs) -> None:
        """Hold owners (None: skipped) that the launches reach only through raw pointers: a descriptor's fields, address + offset."""
        self.keep += [o for o in objs if o is not None]

    def run(self, stream: int, start: int = 0, stop=None) -> None:
        """Launch entries [start, stop) on ``stream`` in order; the first failure raises and nothing behind it is launched."""
        st = C.c_void_p(stream)
        for fn, name, args in self.calls[start:stop]:
            capi.check(fn(*args, st), name)

    def select(self, pred):
        """The entries whose name satisfies ``pred``, in order, as a list that shares ``keep``."""
        out = LaunchList(self.keep)
        out.calls = [c for c in self.calls if pred(c[1])]
        return out

    def names(self):
        return [name for _, name, _ in self.calls]

    def __len__(self) -> int:
        return len(self.calls)

    def __iter__(self):
        return iter(self.calls)

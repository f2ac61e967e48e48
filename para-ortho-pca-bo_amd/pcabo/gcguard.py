"""Keep CPython's cyclic garbage collector out of the BO loop.

With torch and numpy imported a process holds several hundred thousand long-lived container objects.  The loop of a run
allocates a few hundred tracked objects per iteration (tensors, arrays, tuples), which trips the collector's generation
thresholds regularly, and every full collection walks all of those old objects again: measured on the MI355X host as
0.3-0.45 ms per BO iteration (of 3.0-3.6), landing wherever the threshold happens to trip - typically in the torch ops of
the initial pick.  `gc.freeze()` moves everything that exists when a run starts into the permanent generation, so the
collections during the run only see the run's own objects; `gc.unfreeze()` gives the objects back when the last run
ends.  Nothing is leaked and the collector stays enabled.  The optimisers' `gc_freeze=False` switches this off.
"""
from __future__ import annotations

import gc
import threading

_lock = threading.Lock()
_depth = 0
_saved_threshold = None
_YOUNG_THRESHOLD = 50000


def enter() -> None:
    global _depth, _saved_threshold
    with _lock:
        if _depth == 0:
            gc.freeze()
            _saved_threshold = gc.get_threshold()
            gc.set_threshold(max(_saved_threshold[0], _YOUNG_THRESHOLD), *_saved_threshold[1:])
        _depth += 1


def leave() -> None:
    global _depth, _saved_threshold
    with _lock:
        if _depth > 0:
            _depth -= 1
            if _depth == 0:
                if _saved_threshold is not None:
                    gc.set_threshold(*_saved_threshold)
                    _saved_threshold = None
                gc.unfreeze()


class RunGuard:
    """What a run (a single optimiser's, a lock-step batch's) switches on around its loop and off again after it, also after a
    start that failed half-way: torch's intra-op threads capped at `torch_threads` (None: left alone) - torch only serves the Sobol
    / multinomial draws here, and its default of one OpenMP worker per visible core (hundreds on a GPU host) leaves spinning workers
    that starve the host threads driving the device loop (measured: 300 us instead of 34 us per L-BFGS-B round) - and, with
    `gc_freeze`, the collector's guard above.  leave() puts back the thread count from before the run; both calls may be repeated."""

    def __init__(self, torch_threads=4, gc_freeze: bool = True):
        self._torch_threads, self._gc_freeze = torch_threads, bool(gc_freeze)
        self._saved_threads, self._gc_entered = None, False

    def enter(self) -> None:
        if self._torch_threads is not None and self._saved_threads is None:
            import torch
            if torch.get_num_threads() > int(self._torch_threads):
                self._saved_threads = torch.get_num_threads()
                torch.set_num_threads(int(self._torch_threads))
        if self._gc_freeze and not self._gc_entered:
            enter()
            self._gc_entered = True

    def leave(self) -> None:
        if self._gc_entered:
            leave()
            self._gc_entered = False
        if self._saved_threads is not None:
            import torch
            torch.set_num_threads(self._saved_threads)
            self._saved_threads = None

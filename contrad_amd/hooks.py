"""What the training scripts know of one monitoring hook: a ``Hook`` per evaluator module (``knn.HOOK``, ``prdc.HOOK``, ...),
listed once, in evaluation order, by train_driver.py (``HOOKS``), which adds the flags, checks them, builds the monitors on
rank 0 and evaluates them in four loops over that list.  The monitors themselves: evaluate/gan.py's ``WeightsMonitor``."""
from argparse import SUPPRESS
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Callable, Optional


@dataclass(frozen=True, eq=False)
class Hook:
    flags: tuple                            # ((name, default, argparse keywords), ...) in --help order; no leading dashes
    switch: str                             # the flag (P's attribute) that turns the hook on
    build: Callable                         # (H, run) -> the monitor; H: ``check(P)``, run: build_run's ``monitor_run``
    log_lines: Callable                     # (monitor, step, out) -> the lines of log.txt for ``out`` of ``monitor.update``
    shown: str = 'G'                        # whose weights: 'D', or 'G' (g_ema where the script has one)
    needs: str = 'FILE.npz'                 # what the switch takes, for the refusal of its companions without it
    refusals: Optional[Callable] = None     # (H, P): the hook's own device-free refusals (ValueError)
    improved: Optional[Callable] = None     # out -> whether this step's networks are saved as ``*_best.pt`` (PRDC)
    suppressed: bool = True                 # False (kNN): ordinary argparse defaults, and companions without the switch pass

    @property
    def defaults(self):
        return {name: default for name, default, _ in self.flags}

    def add_arguments(self, parser):
        """The flags of the training scripts.  A suppressed flag that is not given leaves no attribute on the parsed
        namespace (read the flags through ``check`` / ``options``): a run without the hook parses to what it parsed to
        before the hook existed."""
        for name, default, kw in self.flags:
            parser.add_argument('--' + name, default=SUPPRESS if self.suppressed else default, **kw)

    def options(self, P):
        """The hook's flags of a parsed command line, defaults filled in."""
        return SimpleNamespace(**{name: getattr(P, name, default) for name, default in self.defaults.items()})

    def on(self, P):
        return bool(getattr(P, self.switch, None))

    def check(self, P):
        """Refusals that need no device (called before the first CUDA call) -> ``options(P)``."""
        H = self.options(P)
        given = [name for name in self.defaults if name != self.switch and hasattr(P, name)]
        if self.suppressed and given and not self.on(P):
            raise ValueError('%s do%s nothing without --%s %s' % (', '.join('--' + g for g in given), 'es' if len(given) == 1 else '',
                                                                 self.switch, self.needs))
        if self.refusals is not None:
            self.refusals(H, P)
        return H

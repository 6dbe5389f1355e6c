"""Process-wide switches and hooks of the operator layer, in ONE object (`STATE`) instead of module globals.

Every op reads its strategy / hook from here at call time, so a caller that wants another setting changes it through
`STATE.override(...)` (restored on exit) or assigns the field — and `STATE.assert_defaults()` tells whether anything was
left changed (tests/conftest.py checks it before every test: the parity suite must run what ships)."""
import contextlib
import os


class OpsState:
    SWITCHES = ('msda_bwd', 'attn_core')  # the strategy fields (the hooks below are not switches)

    def __init__(self):
        self.msda_bwd = os.environ.get('RSCOTR_MSDA_BWD', 'tiled')  # 'tiled' | 'sorted' | 'scatter' (ops/deform.py)
        self.attn_core = True  # dense attention (head dim 32) as one fused pass per direction, no stored scores
        # hooks (None = inactive)
        self.grad_sink = None      # rscotr_amd.optim.FlatAdamW: backward kernels add parameter gradients into its arena
        self.side = None           # active side stream of the weight-gradient contractions (ops.side_enable)
        self.profile = None        # list: every profiled launch appends dict(kind, bytes, e0, e1) (bench.py)
        self.profile_every = {'gemm': 8}
        self._defaults = {name: getattr(self, name) for name in self.SWITCHES}

    def defaults(self):
        """The switch values this process started with (environment or built-in)."""
        return dict(self._defaults)

    def changed(self):
        """{field: (current, default)} of every switch that no longer has its start value."""
        return {k: (getattr(self, k), v) for k, v in self._defaults.items() if getattr(self, k) != v}

    def assert_defaults(self):
        ch = self.changed()
        if ch:
            raise AssertionError(f'operator switches differ from the product defaults: {ch}')

    @contextlib.contextmanager
    def override(self, **kw):
        old = {k: getattr(self, k) for k in kw}
        for k in kw:
            if k not in self.SWITCHES and k not in ('profile', 'side', 'grad_sink'):
                raise AttributeError(k)
        try:
            for k, v in kw.items():
                setattr(self, k, v)
            yield self
        finally:
            for k, v in old.items():
                setattr(self, k, v)


STATE = OpsState()

"""What the bindings of every stage handle share (_lib.STAGES lists them): creation from the stage's config structure, the
handle's lifetime, and the check / status / stream calls, all found from the stage's C prefix."""
import ctypes as C

from . import _lib
from ._lib import check


class StageHandle:
    """Base of a binding of aria_<prefix>_t. A subclass names `_prefix` and `_config` and builds its handle in __init__ with
    cfg = self._default_config(device, stream), its own fields, self._create(cfg)."""

    _prefix = None       # "pose": aria_pose_create, aria_pose_check, ...
    _config = None       # the ctypes structure of aria_<prefix>_config

    def _fn(self, name):
        return getattr(self._L, "aria_%s_%s" % (self._prefix, name))

    def _default_config(self, device, stream):
        self._L = _lib.load_library()
        cfg = self._config()
        self._fn("default_config")(C.byref(cfg))
        cfg.device = device
        cfg.stream = stream
        return cfg

    def _create(self, cfg):
        self.config = cfg
        h = C.c_void_p()
        check(self._fn("create")(C.byref(cfg), C.byref(h)), "aria_%s_create" % self._prefix)
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._fn("destroy")(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self):
        """Synchronise the handle's stream; raise on a deferred error of the device calls (what the stage's kernels refused:
        out-of-range counts or indices, an invalid or too large input, a result cut at the caller's capacity)."""
        check(self.status(), "aria_%s_check" % self._prefix)

    def status(self):
        """aria_<prefix>_check's status code, without raising. Reported once: the next call returns ARIA_OK."""
        return self._fn("check")(self._h)

    @property
    def stream(self):
        return self._fn("stream")(self._h)

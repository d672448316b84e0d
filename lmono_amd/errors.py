"""The package's one exception type (a module of its own so that the numpy-only tools need no ctypes)."""


class LmonoError(RuntimeError):
    """Raised by every entry point; .code carries the C return value where the library gave one."""

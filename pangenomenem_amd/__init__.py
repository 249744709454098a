"""PPanGGOLiN's partitioning on the MI355X.  The loader's names are the package's too (resolved on first use)."""
_LOADER = ("load_files", "load_arrays_host", "Loaded")


def __getattr__(name):
    if name in _LOADER:
        from . import loader
        return getattr(loader, name)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))

"""The compiled reference's answers, recorded: tests that compare against the unmodified reference (oracle/_ref) read
what it returned for the same call from tests/golden/refcalls/ instead of calling it, so they run on any machine.

A call is looked up by a digest of its method, its arguments (arrays by dtype, shape and bytes) and, for ``nem()``,
the content of the input files it reads; what is stored is data only: the returned arrays and scalars and, for
``nem()``, the files it wrote.  tests/golden/make_refcalls.py records them from the compiled reference.
A call the recording does not hold fails the test: its inputs or arguments are not the ones recorded.
Timings of the recording host are not answers and are not kept, except the wall time of a ``nem()`` call
(``recorded_seconds``): a test that times the reference where it runs falls back to it, and says so, only where the
compiled reference is absent."""
import gzip
import hashlib
import inspect
import json
import os
import time

import numpy as np

REFCALLS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refcalls")
NEM_INPUTS = (".str", ".dat", ".nei", ".m")


def _feed(h, v):
    if isinstance(v, np.ndarray):
        a = np.ascontiguousarray(v)
        h.update(("nd:%s:%s;" % (a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    elif isinstance(v, (tuple, list)):
        h.update(b"seq:%d;" % len(v))
        for e in v:
            _feed(h, e)
    elif isinstance(v, bytes):
        h.update(b"b:" + v + b";")
    elif isinstance(v, str):
        h.update(("s:" + v + ";").encode())
    elif v is None:
        h.update(b"none;")
    elif isinstance(v, (bool, np.bool_)):
        h.update(b"bool:%d;" % int(v))
    elif isinstance(v, (int, np.integer)):
        h.update(b"i:%d;" % int(v))
    elif isinstance(v, (float, np.floating)):
        h.update(("f:%s;" % float(v).hex()).encode())
    else:
        raise TypeError("cannot key a %s" % type(v).__name__)


def _key(method, bound):
    h = hashlib.sha256(method.encode() + b";")
    for name, v in bound.items():
        h.update(name.encode() + b"=")
        if method == "nem" and name == "fname":          # the files' content, not where they lie
            base = v.decode() if isinstance(v, bytes) else v
            _feed(h, os.path.basename(base))
            for ext in NEM_INPUTS:
                p = base + ext
                _feed(h, open(p, "rb").read() if os.path.isfile(p) else None)
        else:
            _feed(h, v)
    return method + "_" + h.hexdigest()[:24]


def _save(key, out, files, seconds):
    os.makedirs(REFCALLS, exist_ok=True)
    arrays, scalars = {}, {}
    for name, v in (out or {}).items():
        if isinstance(v, np.ndarray):
            arrays[name] = v
        elif isinstance(v, (bool, np.bool_)):
            scalars[name] = bool(v)
        elif isinstance(v, (int, np.integer)):
            scalars[name] = int(v)
        elif isinstance(v, (float, np.floating)):
            scalars[name] = float(v)
        elif isinstance(v, str):                       # (the reference's log text: latin-1, arbitrary length)
            arrays["str:" + name] = np.frombuffer(v.encode("latin1"), np.uint8)
        else:
            raise TypeError("cannot record %s of type %s" % (name, type(v).__name__))
    meta = dict(scalars=scalars, arrays=sorted(arrays), files=sorted(files))
    if seconds is not None:
        meta["recorded_seconds"] = seconds
    np.savez_compressed(os.path.join(REFCALLS, key + ".npz"), **arrays)
    for ext, data in files.items():
        with gzip.GzipFile(os.path.join(REFCALLS, "%s%s.gz" % (key, ext)), "wb", mtime=0) as f:
            f.write(data)
    with open(os.path.join(REFCALLS, key + ".json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)


def _load(key):
    p = os.path.join(REFCALLS, key + ".json")
    if not os.path.isfile(p):
        raise AssertionError("no recorded reference call %s: the inputs or arguments differ from the recorded ones "
                             "(tests/golden/make_refcalls.py records them)" % key)
    meta = json.load(open(p))
    out = dict(meta["scalars"])
    if meta["arrays"]:
        z = np.load(os.path.join(REFCALLS, key + ".npz"))
        for name in meta["arrays"]:
            if name.startswith("str:"):
                out[name[4:]] = z[name].tobytes().decode("latin1")
            else:
                out[name] = z[name]
    files = {ext: gzip.open(os.path.join(REFCALLS, "%s%s.gz" % (key, ext)), "rb").read() for ext in meta["files"]}
    return out, files, meta.get("recorded_seconds")


def _outputs(base):
    """{extension: (mtime, size)} of the files <base>.* """
    d, stem = os.path.split(base)
    return {name[len(stem):]: (os.stat(os.path.join(d, name)).st_mtime_ns, os.stat(os.path.join(d, name)).st_size)
            for name in os.listdir(d) if name.startswith(stem + ".")}


class RecordedReference:
    """pyoracle.Reference's interface over the recording.  With ``live`` (a pyoracle.Reference) every call goes to the
    compiled reference and is recorded.  ``recorded_seconds``: the wall time the last nem() call took on the host that
    recorded it (None for the other calls) -- not a measurement of the machine running the test."""

    def __init__(self, live=None):
        from oracle import pyoracle
        self._api = pyoracle.Reference
        self.live = live
        self.recorded_seconds = None

    def _call(self, method, args, kwargs):
        sig = inspect.signature(getattr(self._api, method))
        bound = sig.bind(None, *args, **kwargs)
        bound.apply_defaults()
        params = dict(bound.arguments)
        params.pop("self")
        key = _key(method, params)
        if self.live is None:
            out, files, self.recorded_seconds = _load(key)
            if method == "nem":
                base = params["fname"].decode() if isinstance(params["fname"], bytes) else params["fname"]
                for ext, data in files.items():
                    with open(base + ext, "wb") as f:
                        f.write(data)
                return out["rc"]
            return out
        if method == "nem":
            base = params["fname"].decode() if isinstance(params["fname"], bytes) else params["fname"]
            before = _outputs(base)
        t0 = time.perf_counter()
        out = getattr(self.live, method)(*args, **kwargs)
        seconds = time.perf_counter() - t0
        if method == "nem":                              # the files the call wrote
            files = {ext: open(base + ext, "rb").read() for ext, t in _outputs(base).items() if before.get(ext) != t}
            self.recorded_seconds = seconds
            _save(key, dict(rc=out), files, seconds)
        else:                                            # (the reference's own loop time is this host's, not an answer)
            self.recorded_seconds = None
            _save(key, {name: v for name, v in out.items() if name != "seconds"}, {}, None)
        return out

    def nem(self, *args, **kwargs):
        return self._call("nem", args, kwargs)

    def classify(self, *args, **kwargs):
        return self._call("classify", args, kwargs)

    def classify_random(self, *args, **kwargs):
        return self._call("classify_random", args, kwargs)

    def estim_para(self, *args, **kwargs):
        return self._call("estim_para", args, kwargs)

"""Recipe for oracle/_ref/: the reference implementation's `sygnals` package, byte-compiled.

Two CPU tests (tests/test_plugin_cli.py) drive the reference's own PluginRegistry and PluginLoader against this
package's plugin.  No source of the reference is kept in this repository: `__graft_entry__.build()` runs this recipe,
which compiles every module of the reference's `sygnals` package to a sourceless .pyc under oracle/_ref/sygnals/
(importable with oracle/_ref on sys.path, by the interpreter that compiled it).  oracle/_ref/ stays out of git.

The reference checkout is the one named by $SYGNALS_REFERENCE, else by BASELINE.json's `reference_path`.  Where it is
not readable, nothing is built and those two tests skip.

    python -m oracle.build_ref          # or: __graft_entry__.build()
"""
import json
import os
import py_compile
import shutil
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "oracle", "_ref")


def reference_checkout():
    path = os.environ.get("SYGNALS_REFERENCE")
    if not path:
        try:
            path = json.load(open(os.path.join(ROOT, "BASELINE.json"))).get("reference_path")
        except (OSError, ValueError):
            path = None
    return path


def build_ref(quiet=False):
    """Compile the reference's `sygnals` package into oracle/_ref/sygnals/; returns the package directory, or None
    when no readable reference checkout is found (an earlier build is then left as it is)."""
    ref = reference_checkout()
    src = os.path.join(ref, "sygnals") if ref else None
    try:
        readable = bool(src) and os.path.isfile(os.path.join(src, "plugins", "api.py")) and os.access(src, os.R_OK | os.X_OK)
    except OSError:
        readable = False
    if not readable:
        if not quiet:
            print(f"oracle/_ref: no readable reference checkout ({ref!r}); the tests that need it will skip")
        return None
    dst = os.path.join(OUT, "sygnals")
    tmp = dst + ".tmp"
    shutil.rmtree(tmp, ignore_errors=True)
    for d, _, files in os.walk(src):
        for f in sorted(files):
            if not f.endswith(".py"):
                continue
            rel = os.path.relpath(os.path.join(d, f), src)
            out = os.path.join(tmp, rel[:-3] + ".pyc")
            os.makedirs(os.path.dirname(out), exist_ok=True)
            py_compile.compile(os.path.join(d, f), cfile=out, dfile=os.path.join("sygnals", rel), doraise=True)
    shutil.rmtree(dst, ignore_errors=True)
    os.replace(tmp, dst)
    if not quiet:
        print(f"built {os.path.relpath(dst, ROOT)} (python {sys.version_info.major}.{sys.version_info.minor})")
    return dst


if __name__ == "__main__":
    build_ref()

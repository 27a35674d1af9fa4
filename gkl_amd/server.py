"""Start and stop the PairHMM server (gkl_amd/lib/gklhip_server).

One server process per node owns the GPU; client processes (``GKL_HIP_SERVER=PATH``, or
``native.PairHmmContext(server=PATH)`` / ``native.PdhmmContext(server=PATH)``) send it their calls.  ``start`` runs the
server as a fresh child process and waits for its ``ready`` line; ``stop`` sends SIGTERM (the server finishes the calls
in flight, removes the socket and exits 0) and SIGKILL after 10 s.
"""
from __future__ import annotations

import os
import select
import signal
import subprocess
import time
from typing import Optional, Sequence

from .errors import RuntimeException

SERVER_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "gklhip_server")


class ServerHandle:
    """A running server: ``socket_path``, ``proc`` (the subprocess.Popen), ``stats()``, ``pdhmm_stats()``, ``stop()``."""

    def __init__(self, proc: subprocess.Popen, socket_path: str):
        self.proc = proc
        self.socket_path = socket_path

    @property
    def pid(self) -> int:
        return self.proc.pid

    def stats(self) -> dict:
        from . import native
        return native.server_stats(self.socket_path)

    def pdhmm_stats(self) -> dict:
        """The server's PDHMM counters (native.pdhmm_server_stats)."""
        from . import native
        return native.pdhmm_server_stats(self.socket_path)

    def stop(self, timeout: float = 10.0) -> Optional[int]:
        """SIGTERM, then SIGKILL after `timeout` seconds; returns the exit status."""
        if self.proc.poll() is None:
            self.proc.send_signal(signal.SIGTERM)
            try:
                self.proc.wait(timeout)
            except subprocess.TimeoutExpired:
                self.proc.kill()
                self.proc.wait()
        if self.proc.stdout:
            self.proc.stdout.close()
        return self.proc.returncode

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.stop()


def start(socket_path: str, devices: Optional[Sequence[int]] = None, env: Optional[dict] = None,
          timeout: float = 60.0, server_path: Optional[str] = None) -> ServerHandle:
    """Run ``gklhip_server --socket socket_path [--devices ...]`` as a child and wait (at most `timeout` s) for its
    ``ready`` line.  `env`: the server's environment (default: this process's), GKL_HIP_SERVER always removed."""
    exe = server_path or SERVER_PATH
    if not os.path.exists(exe):
        raise RuntimeException(f"{exe} is not built: run `python -c 'import __graft_entry__ as g; g.build()'`")
    cmd = [exe, "--socket", socket_path]
    if devices:
        cmd += ["--devices", ",".join(str(int(d)) for d in devices)]
    e = dict(os.environ if env is None else env)
    e.pop("GKL_HIP_SERVER", None)
    proc = subprocess.Popen(cmd, stdout=subprocess.PIPE, stdin=subprocess.DEVNULL, env=e)
    deadline = time.monotonic() + timeout
    line = b""
    while not line.endswith(b"\n"):
        left = deadline - time.monotonic()
        if left <= 0 or proc.poll() is not None:
            break
        r, _, _ = select.select([proc.stdout], [], [], min(left, 0.5))
        if r:
            b = os.read(proc.stdout.fileno(), 1)
            if not b:
                break
            line += b
    if line.strip() != b"ready":
        if proc.poll() is None:
            proc.kill()
        proc.wait()
        raise RuntimeException(f"PairHMM server on {socket_path} did not become ready (exit status {proc.returncode}, "
                               f"output {line!r})")
    return ServerHandle(proc, socket_path)

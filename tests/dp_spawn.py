"""Starting a gloo world of child processes for a test, so that trouble ends the test instead of hanging it: every child
joins the process group with a 120-second collective timeout; a child that raises prints its traceback and exits non-zero
at once (no interpreter shutdown a peer could wait behind); the parent joins with a limit, fails on the first child that
exits non-zero (torch.multiprocessing terminates its peers) and terminates whatever outlives the limit.  No retries."""
import os
import socket
import sys
import time
import traceback
from datetime import timedelta

import torch.distributed as dist
import torch.multiprocessing as mp


def free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _entry(rank, worker, world, port, args):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        dist.init_process_group("gloo", rank=rank, world_size=world, timeout=timedelta(seconds=120))
        worker(rank, world, *args)
        dist.barrier()
        dist.destroy_process_group()
    except BaseException:
        traceback.print_exc()
        sys.stdout.flush()
        sys.stderr.flush()
        os._exit(1)


def run_world(worker, world, *args, limit: float = 240.0):
    """worker(rank, world, *args) in `world` spawned processes joined in one gloo group; returns when all have exited 0."""
    ctx = mp.spawn(_entry, args=(worker, world, free_port(), args), nprocs=world, join=False)
    deadline = time.monotonic() + limit
    try:
        while not ctx.join(timeout=max(0.1, deadline - time.monotonic())):
            if time.monotonic() >= deadline:
                raise TimeoutError(f"a world of {world} did not finish within {limit:.0f} s")
    finally:
        for p in ctx.processes:
            if p.is_alive():
                p.terminate()
        for p in ctx.processes:
            p.join(10)
            if p.is_alive():
                p.kill()

"""Data-parallel training runs: the sharding rule of the epoch drivers and the rank launcher of the command line.

Standard library only.  The launching process starts one fresh child per GPU and must not have touched a GPU itself, so this file
imports neither torch nor the rest of the package; run as a script (`python neuron-gan_amd/launch.py --gpus N <train flags>`) it
loads the package only in the processes that train (a child, or `--gpus 1`).

Sharding rule: `cfg.batch_size` is the GLOBAL batch of one optimiser step.  Every rank draws the same epoch
permutation `order`; global batch k is order[k*B : (k+1)*B] and rank r trains the slice `shard_bounds(len(batch), world, r)` of it."""
import os
import socket
import subprocess
import sys

MAX_GPUS = 8                    # one node
PKG_NAME = "neuron_gan_amd"


def shard_bounds(b, world, rank):
    """(lo, hi) of rank `rank`'s share of a global batch of b samples: contiguous slices in rank order, the first b % world ranks one
    sample longer"""
    if not (world >= 1 and 0 <= rank < world and b >= 0):
        raise ValueError(f"shard_bounds(b={b}, world={world}, rank={rank})")
    q, r = divmod(b, world)
    lo = rank * q + min(rank, r)
    return lo, lo + q + (1 if rank < r else 0)


def longest_share(b, world):
    """ceil(b / world): rank 0's share, the row count every rank pads gathered per-sample tensors to"""
    return -(-b // world)


def check_sharding(n_images, batch_size, world):
    """Refuse a configuration in which some rank would get an empty slice of some global batch: it would still have to join every
    collective of the step (with zero-count BatchNorm records on the WGAN path)."""
    last = n_images % batch_size if batch_size > 0 else 0
    if n_images < 1 or batch_size < world or 0 < last < world:
        raise ValueError(f"n_images={n_images}, batch_size={batch_size}, world={world}: every rank needs at least one image of every "
                         f"global batch (batch_size >= world, and a last batch of n_images % batch_size = {last} images that is "
                         f"empty or >= world)")


def epoch_batches(order, batch_size, world, rank):
    """[(global batch size, this rank's indices)] of one epoch over the permutation `order`"""
    out = []
    for i in range(0, len(order), batch_size):
        glob = order[i:i + batch_size]
        lo, hi = shard_bounds(len(glob), world, rank)
        out.append((len(glob), glob[lo:hi]))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# launcher
# ---------------------------------------------------------------------------------------------------------------------
def free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def split_gpus(argv):
    """(N, argv without the flag) for `--gpus N` / `--gpus=N` anywhere in argv; N = 1 when absent"""
    n, rest, i = 1, [], 0
    argv = list(argv)
    while i < len(argv):
        a = argv[i]
        if a == "--gpus":
            if i + 1 >= len(argv):
                raise ValueError("--gpus needs a value")
            n, i = int(argv[i + 1]), i + 2
        elif a.startswith("--gpus="):
            n, i = int(a[len("--gpus="):]), i + 1
        else:
            rest.append(a)
            i += 1
    if n < 1:
        raise ValueError(f"--gpus {n}: at least one")
    return n, rest


def visible_gpus(environ=None):
    """Number of GPUs a child could open, found without opening one: the visibility variables the HIP runtime honours, else the
    compute nodes with SIMDs that the kernel driver lists.  None when neither says."""
    environ = os.environ if environ is None else environ
    counts = []
    for var in ("HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES"):
        if var in environ:
            counts.append(len([v for v in environ[var].split(",") if v.strip()]))
    if counts:
        return min(counts)
    nodes = "/sys/class/kfd/kfd/topology/nodes"
    try:
        n = 0
        for d in os.listdir(nodes):
            with open(os.path.join(nodes, d, "properties")) as f:
                props = dict(ln.split()[:2] for ln in f if len(ln.split()) >= 2)
            n += int(props.get("simd_count", "0")) > 0
        return n
    except OSError:
        return None


def launch_plan(n, argv, port=None, environ=None):
    """[(argv_i, env_i)] of the n rank processes of `--gpus n` -- nothing is started.  argv: the training flags (a `--gpus` among them
    is dropped: a rank never launches ranks).  n = 1 yields no plan: the caller trains in its own process, without a process group."""
    n_flag, rest = split_gpus(argv)
    n = n_flag if n is None else int(n)
    if n > MAX_GPUS:
        raise ValueError(f"--gpus {n}: at most {MAX_GPUS} (one node)")
    if n <= 1:
        return []
    seen = visible_gpus(environ)
    if seen is not None and n > seen:
        raise ValueError(f"--gpus {n}: only {seen} GPU(s) visible")
    environ = dict(os.environ if environ is None else environ)
    port = str(port if port is not None else free_port())
    plan = []
    for r in range(n):
        env = dict(environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=port)
        plan.append(([sys.executable, os.path.abspath(__file__)] + rest, env))
    return plan


def launch(plan):
    """Start every process of the plan, wait, return the first non-zero exit status (after terminating the others: they would wait
    for the dead rank in a collective).  A failed rank is not restarted."""
    procs = [subprocess.Popen(a, env=e) for a, e in plan]
    worst = 0
    try:
        for p in procs:
            rc = p.wait()
            if rc != 0 and worst == 0:
                worst = rc
                for q in procs:
                    if q.poll() is None:
                        q.terminate()
    except KeyboardInterrupt:
        for q in procs:
            q.terminate()
        raise
    return worst


def load_package():
    """the directory of this file as the package `neuron_gan_amd` (its name carries a hyphen on disk)"""
    import importlib.util
    if PKG_NAME in sys.modules:
        return sys.modules[PKG_NAME]
    here = os.path.dirname(os.path.abspath(__file__))
    spec = importlib.util.spec_from_file_location(PKG_NAME, os.path.join(here, "__init__.py"), submodule_search_locations=[here])
    mod = importlib.util.module_from_spec(spec)
    sys.modules[PKG_NAME] = mod
    try:
        spec.loader.exec_module(mod)
    except BaseException:
        sys.modules.pop(PKG_NAME, None)
        raise
    return mod


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    n, rest = split_gpus(argv)
    if n > 1 and "RANK" not in os.environ:
        return launch(launch_plan(n, rest))
    load_package().train.main(rest)
    return 0


if __name__ == "__main__":
    sys.exit(main())

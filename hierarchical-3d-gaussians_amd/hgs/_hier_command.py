"""What the hierarchy commands (``python -m hgs.<tool>``) share: the option walk, the read of one ``.hier`` and its
upload, the tail carry, the write, the side files and the exits.  Plain functions; a command keeps
its docstring, ``USAGE``, its table of options, ``parse_args``, its one library call and the sentence it prints."""
from __future__ import annotations

import dataclasses
import os
import shutil
import sys
import time

import torch

SIDE_FILES = ("anchors.bin", "exposure.json")
NAMES = ("xyz", "shs", "alpha", "log_scales", "rots", "nodes", "boxes")     # Hierarchy's fields, write_hierarchy's order
ROWS = NAMES[:5]                                                            # the per-Gaussian ones: G rows each


def walk_args(argv, arity):
    """-> (positionals, seen) or None.  ``arity[name]`` is the number of tokens option ``name`` takes (0: a flag);
    ``seen[name]`` lists its occurrences in order, each a list of raw strings, [] when absent.  The tokens behind an
    option are taken whatever they are; a token that does not start with ``--`` is a positional wherever it stands.
    None for an unknown ``--x`` in option position and for an option with fewer than its tokens left."""
    pos, seen = [], {name: [] for name in arity}
    i = 0
    while i < len(argv):
        a = argv[i]
        if a in arity:
            vals = list(argv[i + 1:i + 1 + arity[a]])
            if len(vals) != arity[a]:
                return None
            seen[a].append(vals)
            i += 1 + arity[a]
        elif a.startswith("--"):
            return None
        else:
            pos.append(a)
            i += 1
    return pos, seen


def require_gpu(tool):
    if not torch.cuda.is_available():
        raise RuntimeError(f"hgs.{tool} works on the GPU; no GPU is visible")


def read_input(tool, in_path):
    """-> (host Hierarchy, N, G, read_s): load_hierarchy timed, behind the GPU check; ValueError unless 1 <= N <= G."""
    from gaussian_hierarchy._C import load_hierarchy
    from .hierarchy import Hierarchy
    require_gpu(tool)
    t0 = time.perf_counter()
    host = Hierarchy(*load_hierarchy(in_path))
    read_s = time.perf_counter() - t0
    N, G = host.num_nodes, int(host.xyz.shape[0])
    if N < 1 or G < N:
        raise ValueError(f"{in_path}: G = {G} rows, N = {N} nodes; 1 <= N <= G expected")
    return host, N, G, read_s


def upload(host, names=NAMES, rows=None):
    """-> a Hierarchy whose tensors ``names`` are on the current device, the per-Gaussian ones cut to their first
    ``rows`` rows (None: all G, a tail included); every other tensor is the host's own.  What goes up is a memory
    decision of each command."""
    dev = torch.device("cuda", torch.cuda.current_device())
    up = lambda k, t: (t[:rows] if rows is not None and k in ROWS else t).to(dev).contiguous()
    return dataclasses.replace(host, **{k: up(k, getattr(host, k)) for k in names})


def with_tail(h, host, N):
    """-> the per-Gaussian tensors of ``h`` on the host, each followed by the host's rows [N:] (the skybox tail)."""
    return [torch.cat([getattr(h, k).cpu(), getattr(host, k)[N:]]) for k in ROWS]


def write_output(out_path, arrays, half=False):
    """Make the output's directory and write_hierarchy ``arrays`` there: a Hierarchy, or its seven tensors in a list or
    tuple; -> write_s."""
    from gaussian_hierarchy._C import write_hierarchy
    t0 = time.perf_counter()
    if not isinstance(arrays, (list, tuple)):
        arrays = [getattr(arrays, k) for k in NAMES]
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    write_hierarchy(out_path, *arrays, half=half)
    return time.perf_counter() - t0


def side_files_beside(in_path):
    in_dir = os.path.dirname(os.path.abspath(in_path))
    return [f for f in SIDE_FILES if os.path.exists(os.path.join(in_dir, f))]


def carry_side_files(in_path, out_path):
    """Copy the side files beside the input to the output's directory unless it is the same; -> (beside, same_dir)."""
    in_dir, out_dir = (os.path.dirname(os.path.abspath(p)) for p in (in_path, out_path))
    beside = side_files_beside(in_path)
    for f in beside:
        if in_dir != out_dir:
            shutil.copyfile(os.path.join(in_dir, f), os.path.join(out_dir, f))
    return beside, in_dir == out_dir


def usage_exit(usage, reason=None) -> int:
    print(usage if reason is None else f"{reason}\n{usage}", file=sys.stderr)
    return 2


def missing_path(tool, *paths) -> bool:
    """Whether one of ``paths`` (None: not given) does not exist; the first such is named on stderr, for the usage exit
    to follow."""
    for path in paths:
        if path is not None and not os.path.exists(path):
            print(f"{tool}: {path} does not exist", file=sys.stderr)
            return True
    return False


def check_exit(tool, sentence) -> int:
    print(f"{tool}: {sentence}; nothing written", file=sys.stderr)
    return 1

"""Op-level access to the native engine primitives.

Everything here dispatches into the in-tree native extension; the HIP
kernels are used automatically when a GPU is visible (Options.gpu="auto"),
and `Options.gpu="force"` makes any silent CPU fallback an error — GPU
tests and the bench run with "force" so a missing/broken kernel fails
loudly instead of quietly passing on the CPU path.
"""

from .. import _core
from .._core import (  # noqa: F401
    combination_rank,
    decode_pair,
    function_lists,
    gen_lut_ttable,
    gen_ttable_2,
    generate_target,
    graph_to_dot,
    graph_to_source,
    lut4s_solve,
    lut5_solve,
    lut7_ordering,
    lut7_solve,
    lut7_solve_ordering,
    make_2_input_fun,
    mask_for_inputs,
    n_choose_k,
    naive_check_n_lut_possible,
    naive_get_lut_function,
    nth_combination,
    pair2_matcher,
    splits5,
    tt_eq_mask,
    ttable_to_string,
)


def make_engine(lut_graph=False, seed=None, gpu="auto", oneoutput=-1,
                iterations=1, metric="gates", try_nots=False,
                save_states=False, output_dir="", verbosity=-1,
                gate_bitfield=None, ctx=None, jobs=1, gpu_pairs="off",
                lut_shared=False, ordered=False):
    """Builds an Engine with the given search options.

    gpu_pairs routes the pair sweeps of gate-mode steps 3 and 4a on an engine
    that has a GPU: "off" keeps the host sweep, "force" sends every sweep
    through the k=2 pair scan, "auto" does so from the measured cutover
    upward. The circuit found is the same under all three.

    lut_shared (LUT mode only) adds the shared-input two-LUT scan between the
    3-LUT and the 5-LUT scan of every node: two LUTs over four gates,
    LUT(LUT(x, y, z), d, s) with s one of x, y, z. Off, the search is
    exactly what it was without the option.

    ordered makes every scan that runs on the GPU report the hit of the
    lowest rank in its window, which is exactly what the CPU scan of that
    window reports (found and res[10]; evaluated is only known to lie in
    [1, window size] on a hit). A seeded search then finds the same circuit
    on every run, under gpu="off", "auto" and "force" alike, and scan_pool /
    scan_shared on the engine inherit the contract. count_all scans ignore
    it; an engine without a GPU accepts it and is unchanged, its scans being
    ordered already. With a ctx of more than one rank the search is
    reproducible for a fixed world and chunk size, but not equal to the
    single-rank search. Off (the default), the GPU scans report whichever
    hit wins their election.
    """
    if lut_shared and not lut_graph:
        raise ValueError("lut_shared needs lut_graph")
    o = _core.Options()
    o.lut_graph = lut_graph
    if seed is not None:
        o.seeded = True
        o.seed = seed
    o.gpu = gpu
    o.gpu_pairs = gpu_pairs
    o.lut_shared = lut_shared
    o.ordered = ordered
    o.oneoutput = oneoutput
    o.iterations = iterations
    o.jobs = jobs
    o.metric = metric
    o.try_nots = try_nots
    o.save_states = save_states
    o.output_dir = output_dir
    o.verbosity = verbosity
    if gate_bitfield is not None:
        o.set_avail_gates(gate_bitfield)
    o.derive_function_lists()
    return _core.Engine(o, ctx)


def scan(engine, k, state, target, mask, begin, end, seed=0, count_all=False,
         excl=0):
    """Runs a 3/5/7-LUT combination scan over [begin, end).

    excl is a bitmask of gate ids < 64 that no reported or counted
    combination may contain (the 3-LUT scan ignores it, as the reference
    does). Returns (found, res[10], evaluated). res layout matches the
    reference's wire format (see sbg/scan.hpp).
    """
    return engine.scan_pool(k, state, target, mask, begin, end, seed, count_all,
                            excl)


def scan_shared(engine, state, target, mask, begin, end, seed=0,
                count_all=False, excl=0):
    """Runs the shared-input two-LUT scan over ranks [begin, end) of C(n, 4).

    A 4-combination hits when LUT(fi; LUT(fo; x, y, z), d, s), with s one of
    x, y, z, realises the target under the mask. Returns (found, res[10],
    evaluated) in the 5-LUT layout: res[0] = fo, res[1] = fi, res[2:5] = the
    outer triple (ascending), res[5] = the rest gate d, res[6] = the shared
    gate, one of res[2:5]. excl and count_all as in scan().
    """
    return engine.scan_shared(state, target, mask, begin, end, seed, count_all,
                              excl)


def scan_pairs(engine, state, target, mask, begin, end, funs="gates",
               order=None):
    """Runs the pair scan (k=2) of gate-mode steps 3 and 4a over ranks
    [begin, end) of C(n, 2), row-major over visit positions i < k.

    Position j holds gate order[j] (a permutation of the pool ids; None is
    the identity). funs picks the engine's function list: "gates", or "not"
    for the NOT-augmented one. Unlike the other scans the result is
    deterministic: the hit of the lowest rank in the window. Returns (found,
    res[10], evaluated) with res[0] = index into the function list, res[1] =
    1 if the arguments are swapped, res[2], res[3] = gate ids in argument
    order; evaluated = hit rank - begin + 1, or the window's size on a miss.
    """
    return engine.scan_pairs(state, target, mask, begin, end, funs, order)

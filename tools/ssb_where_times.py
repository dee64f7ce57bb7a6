#!/usr/bin/env python3
"""The thirteen SSB queries as ONE hy_star_join_aggregate_where call each, timed; and Q2.1 / Q4.1 through hy_star_join_aggregate with two
builds of the library alternating in one process (the acceptance check of the entry point it was generalised from: no slower than before).
Usage: python tools/ssb_where_times.py [sf] [steps]                     the thirteen queries
       python tools/ssb_where_times.py --pairs BASE_LIBRARY [sf] [steps]  four alternating pairs base / this build, Q2.1 and Q4.1, old entry point
Q1.x: the bytes the query has to read (its filter columns, the foreign key and the aggregate's two inputs, each once, as stored) against its time."""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(call, steps):
    """ms per call, after one call that is not counted (a call returns with its result in host memory: nothing is left in flight)"""
    call()
    t0 = time.perf_counter()
    for _ in range(steps):
        call()
    return (time.perf_counter() - t0) / steps * 1e3


def stored_bytes(host_column):
    return sum(segment.data.nbytes for segment in host_column.segments)


def thirteen(sf, steps):
    from hyrise_amd import abi, ssb, storage
    from hyrise_amd.operators import star_join_aggregate_where
    lib = abi.load_library()
    abi.check(lib.hy_init(0))
    lib.hy_debug_star_fused.restype = int
    data = ssb.SsbData(scale_factor=sf, seed=7)
    host = data.host_columns(tables=ssb.SsbData.ALL_TABLES)
    columns = {name: storage.DeviceColumn(column) for name, column in host.items()}
    print(f"SSB SF{sf:g}: {data.n_lineorder} lineorder rows, {steps} steps per query, hy_star_join_aggregate_where")
    for query in ssb.QUERIES:
        dimensions, fact_filters, groupby, aggregates = ssb.star_plan(columns, query, where=True)
        state = {}

        def call():
            state["result"], state["joined"] = star_join_aggregate_where(dimensions, fact_filters, groupby, aggregates, result=state.get("result"))

        ms = timed(call, steps)
        line = f"  Q{query}: {ms:8.3f} ms  {state['joined']:>10} joined rows  {state['result'].n_groups:>4} groups  fused {lib.hy_debug_star_fused()}"
        if not groupby:   # flight 1: what has to be read, once
            names = [name for name, _, _ in ssb.STAR_QUERIES[query][1]] + ["lo_orderdate", "lo_extendedprice"]   # (lo_discount is a filter column and an input)
            read = sum(stored_bytes(host[name]) for name in dict.fromkeys(names))
            line += f"  reads {read / 1e9:.3f} GB ({', '.join(dict.fromkeys(names))}): {read / ms / 1e6:.0f} GB/s"
        print(line, flush=True)


def bind(path):
    """Another build of the library beside the one hyrise_amd loads (its own runtime state; symbols it lacks are left out)."""
    from hyrise_amd import abi
    lib = C.CDLL(path)
    for name, restype, argtypes in abi.SYMBOLS:
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, argtypes
    return lib


def pairs(base_path, sf, steps):
    from hyrise_amd import abi, ssb, storage
    from hyrise_amd.operators import star_join_aggregate
    libraries = {"base": bind(base_path), "new": abi.load_library()}
    data = ssb.SsbData(scale_factor=sf, seed=7)
    host = data.host_columns()
    plans = {}
    for which, lib in libraries.items():   # every build has its own device columns (abi._lib: the build hyrise_amd's calls go to)
        abi._lib = lib
        abi.check(lib.hy_init(0))
        columns = {name: storage.DeviceColumn(storage.HostColumn(column.segments, column.data_type)) for name, column in host.items()}
        plans[which] = {query: ssb.star_plan(columns, query) for query in ("2.1", "4.1")}
    print(f"SSB SF{sf:g}, hy_star_join_aggregate, {steps} steps per run, base = {base_path}")
    print("  pair   Q2.1 base / new (ms)     Q4.1 base / new (ms)")
    for pair in range(4):   # (which build goes first alternates too: whatever the second run of a pair inherits from the first cancels)
        cells = []
        for query in ("2.1", "4.1"):
            ms = {}
            for which in (("base", "new") if pair % 2 == 0 else ("new", "base")):
                abi._lib = libraries[which]
                dimensions, groupby, aggregates = plans[which][query]
                state = {}

                def call():
                    state["result"], state["joined"] = star_join_aggregate(dimensions, groupby, aggregates, result=state.get("result"))

                ms[which] = timed(call, steps)
            cells.append(f"{ms['base']:.4f} / {ms['new']:.4f}")
        print(f"  {pair + 1}      {cells[0]}          {cells[1]}", flush=True)


if __name__ == "__main__":
    arguments = sys.argv[1:]
    if arguments and arguments[0] == "--pairs":
        pairs(arguments[1], float(arguments[2]) if len(arguments) > 2 else 30.0, int(arguments[3]) if len(arguments) > 3 else 50)
    else:
        thirteen(float(arguments[0]) if arguments else 30.0, int(arguments[1]) if len(arguments) > 1 else 20)

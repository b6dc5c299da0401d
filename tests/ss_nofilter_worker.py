"""Worker of tests/test_gpu_key_tables.py::test_unfiltered_hash_kernel_in_a_fresh_process (no tests here): the hash-table SAMPLE_SPACE kernel
WITHOUT its filters, eloc_sample_space_kernel<LEN, CPLX, HASH = true> -- the only user of the paired first probes of LookupSink.  ss_form
selects it only when PYNQS_FILTER_BITS=0, which the library reads once per process, so the parent starts this script as a fresh child with
that variable set.  Asserts pynqs_eloc_sample_space_form(...)[0] == 1 (kSsHash) for every table, runs pynqs_eloc_sample_space_hash and
_hash_flip on the chain tables of tests/key_tables.py (one-, two- and three-word keys, 64 and 256 slots) and on the ordinary "half" tables
of the same shapes, real and complex amplitudes, against tests/ss_exact.py (psi(x) bit-exact: asserted here), and prints one JSON line:
{"kind": [...], "ratios": {"<shape>-<table>-<values>-<form>": [|E_got - E_exact| / bound per walker]}} for the parent to check.

    PYNQS_FILTER_BITS=0 python tests/ss_nofilter_worker.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)


def main() -> int:
    assert os.environ.get("PYNQS_FILTER_BITS") == "0", "start me with PYNQS_FILTER_BITS=0"
    import test_gpu_key_tables as G
    import test_gpu_ss_exact as T

    forms = [f for f in T.FORMS if f.name in ("hash", "hash-flip")]
    kinds, ratios = [], {}

    def run(name, table, nkeys, d, mant, plain, part, values):
        res = G.run_forms(d, forms, mant, plain, part, f"no-filter {name}-{table} {values}")
        for fname, r in res:
            ratios[f"{name}-{table}-{values}-{fname}"] = [float(v) for v in r]

    for name, cap in G.NOFILTER_CHAINS:
        kinds.append(G.form_kind(name, cap // 4)[0])
        assert kinds[-1] == 1, f"{name} chain{cap}: form kind {kinds[-1]}, not the unfiltered hash kernel"
        d = G.chain_device(name, cap)
        for values in G.VALUES:
            plain, part = G.chain_yardstick(name, cap, values)
            run(name, f"chain{cap}", cap // 4, d, G.chain_mantissas(name, cap, values), plain, part, values)
    for name in G.NOFILTER_HALF:
        nk = T.table_keys(name, "half").shape[0]
        kinds.append(G.form_kind(name, nk)[0])
        assert kinds[-1] == 1, f"{name} half: form kind {kinds[-1]}, not the unfiltered hash kernel"
        d = T.device(name, "half")
        for values in G.VALUES:
            plain, part = T.yardstick(name, "half", values, 0)
            run(name, "half", nk, d, T.mantissas(name, "half", values), plain, part, values)
    print(json.dumps({"kind": kinds, "ratios": ratios}))
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""Child process of test_excite_gpu.py: what fdtd_excite_set answers a slab of a decomposed grid and a linked context.  A process of its
own because a slab context takes two streams from the library's process-wide pool and hands them back in another order when it closes,
and the p2p self-test of test_parity_gpu.py, later in the suite's process, is sensitive to which pooled streams its slabs get (their
kernels wait for each other and must not share a hardware queue).  Prints the two messages as JSON.

    python tests/excite_slab_child.py
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    from conftest import pkg
    from excite_cases import main_lists, main_sim
    capi = pkg("_capi")
    lib = capi.load_hip_library()
    lists, dt = main_lists(), main_sim().dt
    said = []
    # a slab of two, then an interior slab of three linked to itself
    for kw, link in ((dict(k0=0, nk=6, rank=0, world=2), False), (dict(k0=4, nk=4, rank=1, world=3, flags=capi.FLAG_LOOPBACK), True)):
        e = capi.Engine(lib, 21, 14, 12, dt, **kw)
        if link:
            capi.link(e, e)
            assert e.schedule_info()["transport"] == "linked"
        try:
            e.set_excite(*lists.args())
            said.append(None)
        except capi.FdtdError as err:
            said.append(str(err))
        e.close()
    print(json.dumps(said))


if __name__ == "__main__":
    main()

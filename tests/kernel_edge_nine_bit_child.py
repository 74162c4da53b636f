"""Child process of test_radix_sort_512_bin_path: the radix sort reads
HS_RS_9BIT once per process, so the 512-bin kernels only run in a process
started with HS_RS_9BIT=1.  Exits 0 when every sort matches cpu_ref."""

import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from hyperspace_amd.ops import cpu_ref, native  # noqa: E402

import kernel_edge_common as kc  # noqa: E402


def main():
    assert os.environ.get("HS_RS_9BIT") == "1"
    assert torch.cuda.is_available() and native.available()
    ext = native.ext()
    # proves the flag took effect in THIS process
    radix, shifts = ext.radix_sort_plan((1 << 26) - 1)
    assert radix == 512 and list(shifts) == [0, 9, 18], (radix, shifts)
    n_sorts = 0
    for lo, hi in kc.NINE_BIT_RANGES:
        for n in (5000, 300_000):
            rng = np.random.default_rng(lo % 13 + hi % 7 + n)
            keys = cpu_ref.normalize_key(torch.from_numpy(
                rng.integers(lo, hi, n, dtype=np.int64)))
            mask = kc.varying_mask(keys)
            radix, shifts = ext.radix_sort_plan(mask)
            assert radix == 512, (hex(mask), radix, shifts)
            kc.check_plan_covers(mask, radix, list(shifts))
            for payload in (torch.arange(n, dtype=torch.int64),
                            torch.arange(n, dtype=torch.int64) + 2**40):
                ck, cp = cpu_ref.stable_sort_u64(keys, payload)
                gk, gp = ext.radix_sort_pairs(keys.cuda(), payload.cuda())
                assert torch.equal(ck, gk.cpu()), (lo, hi, n, "keys")
                assert torch.equal(cp, gp.cpu()), (lo, hi, n, "payload")
                n_sorts += 1
    print(f"nine-bit child: {n_sorts} sorts matched cpu_ref")


if __name__ == "__main__":
    main()

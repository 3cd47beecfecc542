"""Fresh-process half of tests/test_gpu_streams.py::test_first_calls_of_a_process_on_two_threads: two threads, one mm_plan,
and the first compute calls of the process made at the same moment (no warm-up: the kernels' function attributes are still
unset when both threads arrive).  Exit 0 and "first calls ok" when both threads' results equal the serial call made
afterwards bit for bit."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    import torch
    import stream_cases as S
    from test_gpu_streams import bit_equal, run_two_threads
    gpu = torch.device("cuda", 0)
    # first the entries that have no plan to set their kernels' dynamic LDS limit in and do it at their first call, behind
    # the per-device flags of csrc/mm_common.h (the change tail, the row-walking IIR filter, the matrix-pipe resampler);
    # then two that only compute with a shared plan
    for name in ("mfcc_change/clip-resident", "sosfiltfilt_f64/workgroup-per-row", "resample_banded_f32/16000-8000",
                 "mfcc/p4-w16s+own-workspace", "mfcc_modspec/p4-w16s+own-workspace"):
        case = S.BY_NAME[name]
        shared = {}
        prepared = [case.prepare(gpu, shared) for _ in range(2)]
        results = run_two_threads(prepared, 2, warm=False)
        p = prepared[0]
        want = {}
        for k in (0, 1):
            p.fill(k)
            want[k] = [t.clone() for t in p.call()]
        torch.cuda.synchronize()
        for i, res in enumerate(results):
            for k, got in res:
                if not (len(got) == len(want[k]) and all(bit_equal(a, b) for a, b in zip(got, want[k]))):
                    print(f"{name}: thread {i}, data set {k}: differs from the serial call")
                    return 1
    print("first calls ok")
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""Fresh-process half of tests/test_gpu_lomb.py::test_first_calls_of_a_process_on_two_threads: two threads make the first
calls of the process to mm_lombscargle_f64 at the same moment (no warm-up: the code objects are not loaded yet when both
threads arrive).  Exit 0 and "first calls ok" when both threads' results equal the serial call made afterwards bit for
bit."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    import torch
    from test_gpu_streams import bit_equal, run_two_threads
    from test_gpu_lomb import STREAM_CASES
    gpu = torch.device("cuda", 0)
    case = STREAM_CASES[2]
    prepared = [case.prepare(gpu, {}) for _ in range(2)]
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
                print(f"{case.name}: thread {i}, data set {k}: differs from the serial call")
                return 1
    print("first calls ok")
    return 0


if __name__ == "__main__":
    sys.exit(main())

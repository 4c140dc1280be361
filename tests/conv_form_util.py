"""Shape-only descriptors for the launch-form query qd_conv2d_i8_form (include/qdiff_hip.h), which is a pure host function:
fake pointers, no GPU.  TEST INFRASTRUCTURE, shared by test_host_logic.py.

Run as a program it prints, as one JSON object, the forms of the benchmark's hot launches under the environment it was started
with: the library reads QD_WIDE_MINK / QD_WIDE_MINBLK / QD_KGROUPS once per process, and a test process may carry values that
test_hip_kernels.py set at import, so the test of the DEFAULT policy asks a child started without them."""
import ctypes
import json
import os
import sys

FAKE = 0x10000          # a non-null, 16-byte aligned "device pointer": the query follows none

KNOBS = ("QD_WIDE_MINK", "QD_WIDE_MINBLK", "QD_KGROUPS", "QD_SPLITK_TARGET")


def form_case(M_shape, N, k, clens, wbits=4, f16=False, epilogue=0, T=0, heads=8, stride=1):
    """(qd_conv_desc with fake pointers, the ConvCall abi_emulator.conv2d_i8_form reads) of one shape."""
    import torch
    from qdiff import hip
    B, H, W = M_shape
    Ho, Wo = (H + stride - 1) // stride, (W + stride - 1) // stride
    d = hip.ConvDesc()
    d.x = d.w = d.out = FAKE
    d.ldx, d.ldo = sum(clens), N
    d.B, d.H, d.W, d.Ho, d.Wo, d.Cout = B, H, W, Ho, Wo, N
    d.kh = d.kw = k
    d.stride, d.pad_t, d.pad_l = stride, k // 2, k // 2
    d.wbits, d.w_tiled, d.nseg, d.epilogue = wbits, 1, len(clens), epilogue
    d.out_dtype = hip.F16 if f16 else hip.F32
    c0 = 0
    for i, cl in enumerate(clens):
        d.seg[i].c0, d.seg[i].clen, d.seg[i].scale = c0, cl, FAKE
        c0 += cl
    hd = None
    if epilogue:
        d.oq_params, d.oq_min, d.oq_max, d.oq_off = FAKE, 0, 255, 128
    if epilogue in (hip.EPI_HEADS_I8, hip.EPI_HEADS_T_I8):
        hd = dict(H=heads, d=N // heads, T=T, Tpad=T, dpad=(N // heads + 31) // 32 * 32)
        d.hd_H, d.hd_d, d.hd_T, d.hd_Tpad, d.hd_dpad, d.hd_sum = hd["H"], hd["d"], T, T, hd["dpad"], FAKE
    call = hip.ConvCall(B=B, H=H, W=W, Ho=Ho, Wo=Wo, Cout=N, kh=k, kw=k, wbits=wbits, epilogue=epilogue, heads=hd,
                        out=torch.empty(0, dtype=torch.float16 if f16 else torch.float32), segs=[dict(clen=cl) for cl in clens])
    return d, call


def form(lib, d):
    out = (ctypes.c_int32 * 4)()
    rc = lib.qd_conv2d_i8_form(ctypes.byref(d), out)
    assert rc == 0, lib.qd_last_error().decode()
    return tuple(out)


def benchmark_forms():
    """bench.py's default workload: eight images per GPU and guidance = a UNet batch of 16; the 64 x 64 level has 320 channels."""
    from qdiff import hip
    lib = hip.load()
    shapes = dict(conv1x1=((16, 64, 64), 320, 1, [320]),
                  conv3x3=((16, 64, 64), 320, 3, [320]),
                  q_heads=((16, 1, 4096), 320, 1, [320], 4, False, hip.EPI_HEADS_I8, 4096),
                  v_heads=((16, 1, 4096), 320, 1, [320], 4, False, hip.EPI_HEADS_T_I8, 4096),
                  skip_two_segments=((16, 64, 64), 320, 1, [320, 320]),
                  conv3x3_32=((16, 32, 32), 640, 3, [640]))
    return {name: form(lib, form_case(*args)[0]) for name, args in shapes.items()}


if __name__ == "__main__":
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "q-diffusion_amd"))
    print(json.dumps(benchmark_forms()))

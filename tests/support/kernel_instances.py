"""The kernel instances a generated stage library carries -- TEST INFRASTRUCTURE ONLY.  A library has one launcher per operation, whatever rows its model
declares; which rows it takes shows in the trailing pack of its kernel instances."""
import subprocess


def kernel_instances(so):
    """the kernel handles of the library as `nm -C` spells them, without the argument lists: {"stage_eval_kernel<SmUser, false, StageData>", ...}"""
    out = subprocess.run(["nm", "-C", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    return {ln.split(" V void ", 1)[1].split("(", 1)[0] for ln in out.splitlines() if " V void stage_" in ln}


def four(pf, *pack):
    """the instances of the four kernels that call F, with the trailing pack `pack` ("StageTheta", "StageData")"""
    args = ", ".join(("SmUser", "true" if pf else "false") + pack)
    return {"stage_%s_kernel<%s>" % (op, args) for op in ("eval", "merit", "advance", "linesearch")}

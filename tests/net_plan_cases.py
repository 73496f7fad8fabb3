"""The plans tests/test_gpu_net_plans.py executes: one small case per plan STRUCTURE the planner (squeezedet_amd/csrc/net.cpp) emits
over make_net_plans_golden.py's matrix, host-only (no torch.cuda; tests/test_net_plan_cases_host.py checks the list on any machine).

A structure is the tuple of a plan's layer names.  Names tell the launch kinds apart except one pair: the streaming
expand + squeeze launch and the ring-chain launch are both called "<fire>/expand+<next>/squeeze1x1"; which of them a plan holds
shows in sqdet_net_overlap_layer (the first chain launch, -1: none).

A case is (arch, dtype, batch, (h, w), option), arch / dtype / option as make_net_plans_golden names them.  The cases keep to the
smallest inputs that still plan the structure, with batch >= 2 (the batch-slot test rolls the batch) and odd sizes where the
structure allows them; what decides a structure besides the option:
  * an odd width (97x131, 97x333) takes the strip stem, so fire2's squeeze stays out of the stem launch; 130x236 takes it in;
  * the 100000-pixel rule of "fire_fuse" 6 / 10 counts batch x map pixels of a fire module.  fire2 / fire3 run on 1/16 of the input
    pixels (97x333: 25x84 = 2100 per image, 48 images pass 100000); fire4 / fire5 on 1/64 -- at most 81/4225 of them (65x65 -> 9x9,
    the SAME pools round up), so the two structures that keep fire4 / fire5 apart as well need batch x 81 > 100000 at the least:
    1235 images of 65x65, 5.2 M input pixels.  No input under PIXEL_CAP plans them: they are the two cases of OVER_CAP;
  * SqueezeDet+'s expand pairs (conv3x3_pair_eligible) split into two convs by batch and map size: 24 x 96x320 splits fire6-fire8,
    32 x 64x1248 fire9-fire11 as well."""
from tests.golden.make_net_plans_golden import ARCHS, DTYPES, OPTIONS, key_of, matrix, plan_text  # noqa: F401  (one definition, there)

PIXEL_CAP = 2600000          # batch * h * w of a case (the benchmark's 32 x 375 x 1242 is 15 M)
OVER_CAP_LIMIT = 5300000     # ... of the two cases no input under the cap reaches (module docstring): 1235 * 65 * 65 = 5217875


def _opt(name, value):
    (o,) = [o for o in OPTIONS if o is not None and o[:2] == (name, value)]
    return o


def _ff(v):
    return _opt("fire_fuse", v)


ODD, EVEN, WIDE = (97, 131), (130, 236), (97, 333)

CASES = [
    # ---- SqueezeDet float16: 11 structures
    ("squeezedet", "f16", 2, EVEN, None),                     # stem + fire2's squeeze, squeeze-tensor launches, ring chains
    ("squeezedet", "f16", 3, ODD, None),                      # strip stem: conv1+pool1, then fire2/squeeze1x1 on its own
    ("squeezedet", "f16", 3, ODD, _ff(2)),                    # three convs per module
    ("squeezedet", "f16", 2, EVEN, _ff(3)),                   # no streaming fire kernel
    ("squeezedet", "f16", 3, ODD, _ff(3)),
    ("squeezedet", "f16", 3, WIDE, _ff(4)),                   # pools kept apart
    ("squeezedet", "f16", 3, ODD, _ff(5)),                    # one launch per module
    ("squeezedet", "f16", 48, WIDE, _ff(6)),                  # chains on the late maps only: fire2 / fire3 past 100000 pixels
    ("squeezedet", "f16", 1235, (65, 65), _ff(6)),            # ... fire4 / fire5 as well (OVER_CAP)
    ("squeezedet", "f16", 3, ODD, _ff(7)),                    # no whole-module + next-squeeze launch
    ("squeezedet", "f16", 3, ODD, _ff(8)),                    # no expand + squeeze streaming launch: a pooled module ends its run
    ("squeezedet", "f16", 2, EVEN, _ff(9)),                   # fire2's squeeze kept out of the stem launch
    ("squeezedet", "f16", 2, EVEN, _opt("stem_algo", 2)),     # strip stem by option
    ("squeezedet", "f16", 2, EVEN, _opt("stem_algo", 3)),     # (same plan text as the default: another stem kernel under it)
    ("squeezedet", "f16", 3, ODD, _opt("conv_algo", 1)),      # generic kernels only
    # ---- SqueezeDet float32: 5 structures
    ("squeezedet", "f32", 3, ODD, None),
    ("squeezedet", "f32", 2, EVEN, None),
    ("squeezedet", "f32", 3, ODD, _ff(2)),
    ("squeezedet", "f32", 48, WIDE, _ff(10)),                 # the pixel rule: fire3 as three convs
    ("squeezedet", "f32", 1235, (65, 65), _ff(10)),           # ... fire4 / fire5 as well (OVER_CAP)
    ("squeezedet", "f32", 3, ODD, _opt("conv_algo", 1)),
    # ---- SqueezeDet+ float16: 11 structures
    ("squeezedet_plus", "f16", 3, ODD, None),
    ("squeezedet_plus", "f16", 3, ODD, _ff(2)),
    ("squeezedet_plus", "f16", 3, ODD, _ff(5)),
    ("squeezedet_plus", "f16", 3, ODD, _ff(11)),              # no pair launch
    ("squeezedet_plus", "f16", 3, ODD, _opt("conv_algo", 1)),
    ("squeezedet_plus", "f16", 24, (96, 320), None),          # fire6-fire8 as three convs
    ("squeezedet_plus", "f16", 24, (96, 320), _ff(5)),
    ("squeezedet_plus", "f16", 24, (64, 1248), _ff(10)),
    ("squeezedet_plus", "f16", 32, (64, 1248), None),         # fire9-fire11 as three convs, too
    ("squeezedet_plus", "f16", 32, (64, 1248), _ff(6)),
    ("squeezedet_plus", "f16", 32, (64, 1248), _ff(10)),
    # ---- SqueezeDet+ float32: 2 structures
    ("squeezedet_plus", "f32", 3, ODD, None),
    ("squeezedet_plus", "f32", 3, ODD, _opt("conv_algo", 1)),
    # ---- ResNet50: 2 structures per dtype (the fused stem or not)
    ("resnet50", "f16", 3, ODD, None),
    ("resnet50", "f16", 3, ODD, _opt("conv_algo", 1)),
    ("resnet50", "f32", 3, ODD, None),
    ("resnet50", "f32", 3, ODD, _opt("conv_algo", 1)),
    # ---- VGG16: 2 structures per dtype (conv + pool in one launch or not)
    ("vgg16", "f16", 2, ODD, None),
    ("vgg16", "f16", 2, ODD, _opt("conv_pool", 0)),
    ("vgg16", "f16", 2, ODD, _opt("conv_algo", 1)),
    ("vgg16", "f32", 2, ODD, None),
    ("vgg16", "f32", 2, ODD, _opt("conv_pool", 0)),
]

OVER_CAP = [c for c in CASES if c[2] * c[3][0] * c[3][1] > PIXEL_CAP]

ARCH_ID = dict(ARCHS)
DTYPE_ID = dict(DTYPES)


def case_id(case):
    return key_of(*case)


def case_text(lib, case):
    """plan_text of a case."""
    arch, dtype, batch, size, option = case
    return plan_text(lib, ARCH_ID[arch], DTYPE_ID[dtype], batch, size, option)


def names_of(text):
    return tuple(line.split(" ")[1] for line in text.split("\n") if line.startswith("layer "))


def structure(lib, arch, dtype, batch, size, option):
    """The plan's layer names in launch order; arch / dtype as names ("squeezedet", "f16") or as the library's ids."""
    return names_of(plan_text(lib, ARCH_ID.get(arch, arch), DTYPE_ID.get(dtype, dtype), batch, size, option))

"""CPU test of the ctypes mirrors of the header's structs: a C program compiled against include/os2s.h prints
sizeof and offsetof of every field, and each mirror in capi.py has the same field names in the same order,
the same offsets and the same size."""
import ctypes
import os
import re
import shutil
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "os2s.h")


def _mirrors():
  from openseq2seq_amd import capi
  return {"os2s_conv_group_t": capi._ConvGroup, "os2s_dres_seg_t": capi._DresSeg,
          "os2s_cwgrad_group_t": capi._CWgradGroup, "os2s_wgrad_group_t": capi._WgradGroup,
          "os2s_opt_config_t": capi.OptConfig, "os2s_rnn_dir_fwd_t": capi._RnnDirFwd,
          "os2s_rnn_dir_bwd_t": capi._RnnDirBwd, "os2s_attn_decoder_t": capi._AttnDecoder,
          "os2s_attn_decoder_grads_t": capi._AttnDecoderGrads, "os2s_tacotron_infer_t": capi._TacotronInfer}


def _header_fields(typedef):
  """Field names of `typedef struct [tag] { ... } typedef;` in declaration order."""
  from openseq2seq_amd import _lib
  text = _lib.strip_comments(open(HEADER).read())
  body = re.search(r"typedef struct\s*\w*\s*\{([^{}]*)\}\s*%s\s*;" % typedef, text).group(1)
  names = []
  for decl in body.split(";"):
    for d in decl.split(","):
      if d.strip():
        names.append(re.search(r"(\w+)\s*(\[[^\]]*\])?\s*$", d).group(1))
  return names


def _compiler():
  for cc in (shutil.which("cc"), "/opt/rocm/llvm/bin/clang"):
    if cc and os.path.exists(cc):
      return cc
  raise AssertionError("no C compiler (cc or ROCm's clang) to check the struct layouts with")


def test_struct_mirrors_match_the_header_layout(tmp_path):
  mirrors = _mirrors()
  fields = {t: _header_fields(t) for t in mirrors}
  lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "os2s.h"', "int main(void) {"]
  for t, names in fields.items():
    lines.append('  printf("%s sizeof %%zu\\n", sizeof(%s));' % (t, t))
    lines += ['  printf("%s %s %%zu\\n", offsetof(%s, %s));' % (t, n, t, n) for n in names]
  lines += ["  return 0;", "}"]
  src, exe = tmp_path / "layout.c", tmp_path / "layout"
  src.write_text("\n".join(lines) + "\n")
  subprocess.run([_compiler(), "-std=c99", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)],
                 check=True)
  c = {}
  for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
    t, field, value = line.split()
    c[t, field] = int(value)
  for t, S in mirrors.items():
    assert [f[0] for f in S._fields_] == fields[t], t
    assert ctypes.sizeof(S) == c[t, "sizeof"], t
    for name in fields[t]:
      assert getattr(S, name).offset == c[t, name], (t, name)

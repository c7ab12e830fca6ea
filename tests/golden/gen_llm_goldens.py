#!/usr/bin/env python
"""Record the host-side golden data of the LLM stage FROM THE REFERENCE'S OWN FILES into llm_host.json (data only):

  prompts   `conv_templates['vicuna_v1']` with one user turn and an open assistant turn (instructany2pix/llm/conversation.py, loaded by path
            as a module: it imports the standard library only), for the instructions listed below
  stop_str  the stop string `forward_llm` derives from that template (pipeline.py:183)
  objs      `InstructAny2PixPipeline.get_all_objs` (pipeline.py:281-287, cut out of the file by AST: the module imports packages that are
            not installed here) on generated-text samples

    python tests/golden/gen_llm_goldens.py <path of the reference checkout>
"""
import ast
import importlib.util
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))

INSTRUCTIONS = ["turn the fox blue", "add [image1] to [image0] and make it sound like [audio2]", ""]
TEXTS = [
    "<s> USER: x ASSISTANT: [a blue fox] <base> <video> <im_gen> <video> additions: fox:<video>, snow:<video></s>",
    "<s> USER: x ASSISTANT: [a blue fox] <im_gen> <video></s>",
    "<s> USER: x ASSISTANT: [two dogs] <im_gen> <video> additions: the left dog:<video></s>",
    "<s> USER: x ASSISTANT: [a cat] <im_gen> <video> additions: cat:<video>",
]


def main(ref):
    spec = importlib.util.spec_from_file_location("ref_conversation", os.path.join(ref, "instructany2pix/llm/conversation.py"))
    conv_mod = importlib.util.module_from_spec(spec)
    sys.modules["ref_conversation"] = conv_mod
    spec.loader.exec_module(conv_mod)
    prompts = []
    for inst in INSTRUCTIONS:
        conv = conv_mod.conv_templates["vicuna_v1"].copy()
        conv.append_message(conv.roles[0], inst)
        conv.append_message(conv.roles[1], None)
        prompts.append({"inst": inst, "prompt": conv.get_prompt()})
    conv = conv_mod.conv_templates["vicuna_v1"].copy()
    stop_str = conv.sep if conv.sep_style != conv_mod.SeparatorStyle.TWO else conv.sep2

    relpath = "instructany2pix/pipeline.py"
    tree = ast.parse(open(os.path.join(ref, relpath)).read())
    ns = {"re": re}
    for node in ast.walk(tree):
        if isinstance(node, ast.ClassDef) and node.name == "InstructAny2PixPipeline":
            for sub in node.body:
                if isinstance(sub, ast.FunctionDef) and sub.name == "get_all_objs":
                    sub.decorator_list = []
                    exec(compile(ast.Module(body=[sub], type_ignores=[]), relpath, "exec"), ns)
    objs = [{"text": t, "objs": ns["get_all_objs"](t)} for t in TEXTS]
    out = {"prompts": prompts, "stop_str": stop_str, "objs": objs}
    with open(os.path.join(HERE, "llm_host.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])

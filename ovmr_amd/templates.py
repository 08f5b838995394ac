"""Prompt templates of the zero-shot trainers (trainers/zsclip.py:13-29, trainers/imagenet_templates.py:86-94).

`ZeroshotCLIP` formats each class name into its dataset's one template; `ZeroshotCLIP2` ensembles the seven
IMAGENET_TEMPLATES_SELECT templates and, on every dataset but ImageNet, the dataset's own template as an eighth (:82-83).
The reference appends that eighth template to the CLASS attribute (`self.templates += [...]`), so a second build in the same process
would see nine; `templates_for` returns a new list every time instead.
"""
from __future__ import annotations

from typing import List

# CUSTOM_TEMPLATES, trainers/zsclip.py:13-29
DATASET_TEMPLATES = {
    "OxfordPets": "a photo of a {}, a type of pet.",
    "OxfordFlowers": "a photo of a {}, a type of flower.",
    "FGVCAircraft": "a photo of a {}, a type of aircraft.",
    "DescribableTextures": "{} texture.",
    "EuroSAT": "a centered satellite photo of {}.",
    "StanfordCars": "a photo of a {}.",
    "Food101": "a photo of {}, a type of food.",
    "SUN397": "a photo of a {}.",
    "Caltech101": "a photo of a {}.",
    "UCF101": "a photo of a person doing {}.",
    "ImageNet": "a photo of a {}.",
    "ImageNetSketch": "a photo of a {}.",
    "ImageNetV2": "a photo of a {}.",
    "ImageNetA": "a photo of a {}.",
    "ImageNetR": "a photo of a {}.",
}

# trainers/imagenet_templates.py:86-94 (the 80-template IMAGENET_TEMPLATES list is not used: the reference leaves it commented out, :67)
IMAGENET_TEMPLATES_SELECT = (
    "itap of a {}.",
    "a bad photo of the {}.",
    "a origami {}.",
    "a photo of the large {}.",
    "a {} in a video game.",
    "art of the {}.",
    "a photo of the small {}.",
)

ZEROSHOT_TRAINERS = ("ZeroshotCLIP", "ZeroshotCLIP2")


def check_dataset(dataset_name: str) -> str:
    """The reference looks the name up in CUSTOM_TEMPLATES and fails with a bare KeyError; here the message lists the known names."""
    if dataset_name not in DATASET_TEMPLATES:
        raise KeyError(f"DATASET.NAME {dataset_name!r} has no zero-shot prompt template (trainers/zsclip.py:13-29); "
                       f"known datasets: {', '.join(sorted(DATASET_TEMPLATES))}")
    return dataset_name


def templates_for(trainer: str, dataset_name: str) -> List[str]:
    """ZeroshotCLIP: [the dataset's template] (:42).  ZeroshotCLIP2: the 7 IMAGENET_TEMPLATES_SELECT on ImageNet, those plus the
    dataset's template (8) on any other dataset (:68, :82-83).  A new list on every call."""
    check_dataset(dataset_name)
    if trainer == "ZeroshotCLIP":
        return [DATASET_TEMPLATES[dataset_name]]
    if trainer == "ZeroshotCLIP2":
        out = list(IMAGENET_TEMPLATES_SELECT)
        if dataset_name != "ImageNet":
            out.append(DATASET_TEMPLATES[dataset_name])
        return out
    raise ValueError(f"unknown zero-shot trainer {trainer!r}; expected one of {ZEROSHOT_TRAINERS}")


def prompts(template: str, classnames) -> List[str]:
    """`temp.format(c.replace("_", " "))` for every class name (:43, :90)."""
    return [template.format(c.replace("_", " ")) for c in classnames]
